"""The checker of the similarity error (tests/_simerr_oracle.py) against a second route in plain Python integers and exact
rationals, on the planted degenerate cases, and as an estimator: the standard error it gives means what the documents say."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import _simerr_cases as cases
from tests import _simerr_oracle as orc


def ulps(got, exact):
    """|got - exact| in units of the last place of got, against an exact rational."""
    return abs(Fraction(got) - exact) / Fraction(math.ulp(got))


TINY = [  # (seed, run lengths, K, N, b)
    (7200, (12,), 2, 6, 3), (7201, (7, 12), 3, 5, 2), (7202, (4, 9, 5), 1, 6, 4), (7203, (12, 11), 2, 4, 1), (7204, (10, 10), 3, 6, 5),
]


@pytest.mark.parametrize("seed,lengths,k,n,b", TINY)
def test_the_moments_equal_plain_python_integers_over_loops(seed, lengths, k, n, b):
    runs = [cases.overlapping(s, k, n, seed=seed + 10 * r, density=0.45) for r, s in enumerate(lengths)]
    s1, s2, nb = orc.moments(runs, b)
    w1, w2, wb = orc.moments_loops([r.tolist() for r in runs], b)
    assert nb == wb == sum(s // b for s in lengths) and s1.dtype == s2.dtype == np.int64
    assert s1.tolist() == w1 and s2.tolist() == w2
    assert np.array_equal(s1, s1.T) and (orc.variance(s1, s2, nb) >= 0).all()
    if all(s % b == 0 for s in lengths):                        # every sample is in a batch: S1 is the similarity count
        z = np.concatenate([r.reshape(-1, n) for r in runs]).astype(np.int64)
        assert np.array_equal(s1, z.T @ z)


@pytest.mark.parametrize("seed,lengths,k,n,b", TINY)
def test_z2_is_within_two_ulp_of_the_exact_rational(seed, lengths, k, n, b):
    side_a = orc.moments([cases.disjoint(s, k, n, seed=seed + 100 + r) for r, s in enumerate(lengths)], b)
    side_b = orc.moments([cases.overlapping(3 * b, k, n, seed=seed + 200, density=0.5)], b)
    z, row_max, row_arg, row_count = orc.compare(side_a, side_b, cases.THRESHOLDS)
    finite = 0
    for i in range(n):
        for j in range(n):
            exact = orc.z2_fraction(int(side_a[0][i, j]), int(side_a[1][i, j]), side_a[2], int(side_b[0][i, j]), int(side_b[1][i, j]), side_b[2])
            if exact == "inf":
                assert z[i, j] == math.inf
            elif exact == 0:
                assert z[i, j] == 0.0
            else:
                finite += 1
                assert ulps(float(z[i, j]), exact) <= 2, (i, j, z[i, j], exact)
    assert finite > n
    assert np.array_equal(z, z.T) and np.array_equal(row_max, z.max(axis=1))
    assert all(z[i, row_arg[i]] == row_max[i] and not (z[i, :row_arg[i]] == row_max[i]).any() for i in range(n))
    assert row_count.tolist() == [[int((z[i] > t).sum()) for t in cases.THRESHOLDS] for i in range(n)]


def test_the_planted_cases():
    b, nb = 4, 3
    run_a, run_b = cases.planted(b, nb)
    side_a, side_b = orc.moments([run_a], b), orc.moments([run_b], b)
    va, vb = orc.variance(*side_a), orc.variance(*side_b)
    # a pair together in exactly one batch: counts (0, b, 0)
    assert side_a[0][4, 7] == b and side_a[1][4, 7] == b * b and va[4, 7] == nb * b * b - b * b and side_b[0][4, 7] == 0 and vb[4, 7] == 0
    # the all-zeros object and the all-ones object: no spread
    assert not side_a[0][3].any() and not va[3].any() and side_a[0][4, 4] == 2 * nb * b and va[4, 4] == 0 and va[4, 0] == 0
    z, row_max, row_arg, row_count = orc.compare(side_a, side_b, (0.0, math.inf))
    assert va[0, 1] == vb[0, 1] == 0 and side_a[0][0, 1] == side_b[0][0, 1] == nb * b and z[0, 1] == 0.0       # V = 0 twice, equal P
    assert va[0, 2] == vb[0, 2] == 0 and side_a[0][0, 2] == nb * b and side_b[0][0, 2] == 0 and z[0, 2] == math.inf   # ... different P
    assert z[0, 8] == math.inf and row_max[0] == math.inf and row_arg[0] == 2                                   # tied maxima: the smallest j
    assert z[3].tolist() == [0.0] * 9 and row_arg[3] == 0 and row_count[3].tolist() == [0, 0]                   # a row of zeros: column 0
    assert 0.0 < z[4, 7] < math.inf and z[4, 7] == (b * nb) ** 2 / ((2.0 * b * b * nb * nb) / (nb - 1))
    assert np.array_equal(z[:, 5], z[:, 6]) and 0.0 < z[4, 5] < math.inf                                        # objects 5 and 6 move as one
    assert row_count[0].tolist() == [int((z[0] > 0.0).sum()), 0]                                                # nothing is above inf
    with pytest.raises(ValueError, match="1 complete batches"):
        orc.moments([run_a[:2 * b - 1]], b)


def mean_ratio(run, b):
    """The mean over the pairs i < j of se^2 / (P (1 - P) / T): 1 for independent samples, the chain's autocorrelation factor
    otherwise."""
    s1, s2, nb = orc.moments([run], b)
    t = nb * b
    p = orc.probability(s1, nb, b)
    upper = np.triu_indices(s1.shape[0], 1)
    return float(np.mean(orc.se_squared(s1, s2, nb, b)[upper] / (p[upper] * (1.0 - p[upper]) / t)))


def test_independent_samples_have_the_binomial_error():
    assert 0.9 < mean_ratio(cases.independent(4096, 3, 40, seed=7300), 64) < 1.1


def test_a_sticky_chain_has_a_larger_error():
    # each object keeps its label with probability 0.9: a pair's indicator has autocorrelation 0.81 per step, (1 + 0.81) / (1 - 0.81) = 9.5
    assert mean_ratio(cases.sticky(4096, 3, 40, seed=7301), 64) > 5.0


def test_two_independent_runs_rarely_pass_the_threshold():
    sides = [orc.moments([cases.independent(4096, 3, 40, seed=7302 + r)], 64) for r in range(2)]
    z = orc.z2(*sides)
    upper = np.triu_indices(40, 1)
    assert float(np.mean(z[upper] > 3.84)) < 0.15


def test_five_objects_forced_together_in_one_run_stand_out():
    run_a, run_b = cases.independent(4096, 3, 40, seed=7304), cases.independent(4096, 3, 40, seed=7305)
    run_b[:, :, 1:5] = run_b[:, :, :1]                          # objects 0 .. 4 share object 0's area in run b
    z = orc.z2(orc.moments([run_a], 64), orc.moments([run_b], 64))
    assert all(z[i, j] > 100.0 for i in range(5) for j in range(5) if i != j)


def test_the_one_call_helpers_of_the_checker():
    runs = [cases.overlapping(s, 2, 7, seed=7400 + s) for s in (37, 50)]
    assert orc.default_batch_rows(runs, 0.0) == 6 and orc.default_batch_rows(runs, 0.1) == 5      # floor(sqrt(37)), floor(sqrt(34))
    kept = orc.trim(runs, 0.1, 5)
    assert [len(r) for r in kept] == [30, 45] and np.array_equal(kept[0], runs[0][7:]) and np.array_equal(kept[1], runs[1][5:])
    best, (i, j), shares, max_abs, object_max = orc.run_agreement(kept, 5, cases.THRESHOLDS)[0, 1]
    z = orc.z2(orc.moments([kept[0]], 5), orc.moments([kept[1]], 5))
    assert best == z.max() == z[i, j] and i <= j and object_max.tolist() == z.max(axis=1).tolist()
    assert shares == [sum(z[p, q] > t for p in range(7) for q in range(p, 7)) / 28 for t in cases.THRESHOLDS]
    pa = orc.probability(orc.moments([kept[0]], 5)[0], 6, 5)
    pb = orc.probability(orc.moments([kept[1]], 5)[0], 9, 5)
    assert abs(max_abs - np.abs(pa - pb).max()) < 1e-12
