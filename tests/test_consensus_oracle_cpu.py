"""The checker of the consensus unit against itself (tests/_consensus_oracle.py): its two forms of the score agree,
Binder's identity holds, and similarity and scores have the symmetries that make them label free.  All in exact integers."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _consensus_cases as cases
from tests import _consensus_oracle as orc


def test_the_two_forms_of_the_score_agree_and_binders_identity_holds():
    c = cases.disjoint(37, 3, 45, seed=4100)
    counts, t = orc.similarity([c])
    assert t == 37 and counts.dtype == np.int64 and np.array_equal(counts, counts.T)
    assert np.array_equal(np.diag(counts), c.any(axis=1).sum(axis=0))        # how often an object is in any area
    by_definition = orc.scores(c, counts, t)
    assert np.array_equal(by_definition, orc.scores_gram(c, [c]))
    assert np.array_equal(by_definition, orc.scores_gather(c, counts, t))
    square = int((counts * counts).sum())
    for s in range(37):
        assert orc.binder_scaled(c[s], counts, t) == t * int(by_definition[s]) + square
    binder = [orc.binder_scaled(sample, counts, t) for sample in c]
    assert orc.consensus([by_definition]) == (0, int(np.argmin(binder)))     # the least-squares sample


def test_the_forms_agree_for_overlapping_rows_and_for_samples_outside_the_selection():
    runs = [cases.overlapping(19, 4, 33, seed=4200 + r) for r in range(3)]
    counts, t = orc.similarity(runs[:2])
    assert t == 38
    for run in runs:                                                        # (run 2 is not part of the matrix)
        want = orc.scores(run, counts, t)
        assert np.array_equal(want, orc.scores_gram(run, runs[:2])) and np.array_equal(want, orc.scores_gather(run, counts, t))


def test_overlapping_rows_follow_the_definition_term_by_term():
    c = cases.overlapping(5, 3, 7, seed=4300, density=0.5)
    assert c.sum(axis=1).max() > 1                                          # an object in two areas of one sample
    counts, t = orc.similarity([c])
    want = [[sum(int(c[s, k, i]) * int(c[s, k, j]) for s in range(5) for k in range(3)) for j in range(7)] for i in range(7)]
    assert counts.tolist() == want
    for s in range(5):
        score = sum(int(c[s, k, i]) * int(c[s, k, j]) * (t - 2 * want[i][j]) for k in range(3) for i in range(7) for j in range(7))
        assert int(orc.scores(c, counts, t)[s]) == score
    empty = np.zeros((1, 3, 7), dtype=np.uint8)
    assert orc.scores(empty, counts, t).tolist() == [0] == orc.scores_gather(empty, counts, t).tolist()
    ones = np.ones((1, 3, 7), dtype=np.uint8)
    assert int(orc.scores(ones, counts, t)[0]) == 3 * (49 * t - 2 * int(counts.sum()))


@pytest.mark.parametrize("tag", ["k3_n100", "k5_n33"])
def test_permuting_every_samples_labels_changes_nothing(tag):
    logged, realigned = cases.golden_realign()[tag]
    assert logged.shape == realigned.shape and not np.array_equal(logged, realigned)
    assert np.array_equal(np.sort(logged.sum(axis=2), axis=1), np.sort(realigned.sum(axis=2), axis=1))      # the same rows, moved
    a, b = orc.similarity([logged]), orc.similarity([realigned])
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
    assert np.array_equal(orc.scores(logged, *a), orc.scores(realigned, *a))
    assert orc.consensus([orc.scores(logged, *a)]) == orc.consensus([orc.scores(realigned, *b)])


def test_permuting_the_objects_permutes_the_matrix():
    c = cases.overlapping(23, 3, 40, seed=4400)
    p = np.random.default_rng(4401).permutation(40)
    counts, t = orc.similarity([c])
    moved, _ = orc.similarity([c[:, :, p]])
    assert np.array_equal(moved, counts[np.ix_(p, p)])
    assert np.array_equal(orc.scores(c[:, :, p], moved, t), orc.scores(c, counts, t))


def test_the_planted_blocks_are_the_consensus_of_their_noisy_samples():
    k, n = 3, 100
    c, _ = cases.planted(k, n, 48, flip=0.05, seed=4500, empty_every=0)
    truth, _ = cases.planted(k, n, 1, flip=0.0, seed=4501, empty_every=0)    # the blocks themselves, rows shuffled
    c[17] = truth[0]
    counts, t = orc.similarity([c])
    scores = orc.scores(c, counts, t)
    assert orc.consensus([scores]) == (0, 17)
    probability = counts / t
    inside = (truth[0].T @ truth[0]).astype(bool)
    assert probability[inside].min() > 0.5 > probability[~inside].max()      # the matrix itself shows the blocks


def test_ties_take_the_smallest_run_and_sample():
    assert orc.consensus([np.array([5, 3, 3]), np.array([3, 9])]) == (0, 1)
    assert orc.consensus([np.array([5, 4]), np.array([3, 3])]) == (1, 0)
    assert orc.consensus([np.array([], dtype=np.int64), np.array([7])]) == (1, 0)
    c = cases.disjoint(9, 3, 20, seed=4600)
    runs = [c, c[::-1].copy()]                                              # every sample twice: once per run
    counts, t = orc.similarity(runs)
    scores = [orc.scores(r, counts, t) for r in runs]
    run, sample = orc.consensus(scores)
    assert run == 0 and sample == int(np.argmin(scores[0])) and scores[1].min() == scores[0].min()


def test_comparison_of_two_matrices():
    a, b = cases.overlapping(12, 3, 9, seed=4700), cases.overlapping(7, 3, 9, seed=4701)
    (ca, ta), (cb, tb) = orc.similarity([a]), orc.similarity([b])
    row_max, row_sum = orc.compare(ca, ta, ca, ta)
    assert not row_max.any() and not row_sum.any()
    row_max, row_sum = orc.compare(ca, ta, cb, tb)
    diff = [[abs(Fraction(int(ca[i, j]), ta) - Fraction(int(cb[i, j]), tb)) for j in range(9)] for i in range(9)]
    assert [Fraction(int(v), ta * tb) for v in row_max] == [max(row) for row in diff]
    assert [Fraction(int(v), ta * tb) for v in row_sum] == [sum(row) for row in diff]
    mx, mean = orc.compare_floats(ca, ta, cb, tb)
    assert mx == float(max(max(row) for row in diff)) and mean == float(sum(sum(row) for row in diff) / 81)
    max_abs, mean_abs = orc.compare_runs([a, b, a])
    assert max_abs[0, 2] == 0.0 == mean_abs[2, 0] and max_abs[0, 1] == max_abs[1, 2] == mx and mean_abs[1, 0] == mean
