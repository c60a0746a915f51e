"""The checker of the power-scaling sensitivity (tests/_psens_oracle.py) pinned on its own: a closed form, a 50-digit evaluation
of its sums, the invariances of the distance, a conjugate case of known order and PSIS by construction."""
import math

import numpy as np
import pytest

from tests import _elpd_oracle as eorc
from tests import _psens_cases as cases
from tests import _psens_oracle as orc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _d(x, w):
    res = orc.column(x, w)
    return orc.distance(res["js"], res["bound"])


def test_the_literal_is_half_over_ln_2():
    assert orc.HALF_INV_LN2 == 0.5 / math.log(2.0)


def test_the_stated_order_of_the_prefix_sum():
    """N = 600: chunks of 3.  Place 4 is the second of chunk 1: (q0 + q1 + q2) + (q3 + q4), over ((c0 + c1) + ..)."""
    q = cases.weights(1, 600, 5)[0]
    big_q, total = orc.prefix_q(q)
    totals = [(q[3 * t] + q[3 * t + 1]) + q[3 * t + 2] for t in range(200)]
    run = 0.0
    for c in totals:
        run = run + c
    assert total == run
    assert big_q[4] == (((q[0] + q[1]) + q[2]) + (q[3] + q[4])) / total
    assert big_q[2] == ((q[0] + q[1]) + q[2]) / total and big_q[599] == 1.0
    assert np.allclose(big_q, np.cumsum(q) / q.sum(), rtol=1e-13, atol=0)
    assert orc.chunk_len(256) == 1 and orc.chunk_len(257) == 2 and orc.depth(1000) == 13


def test_the_tree_is_the_unit_layer_tree():
    v = cases.values(256, 9)
    lanes = v.reshape(4, 64)
    want = []
    for w in range(4):
        a = lanes[w].copy()
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[np.arange(64) ^ o]
        want.append(a[0])
    assert orc.tree(v) == ((want[0] + want[1]) + want[2]) + want[3]


def test_the_closed_form_of_a_binary_column():
    """One gap, at P = 1/2 and Q = 1/4: d = sqrt((P (log2 P - log2 3/8) + Q (log2 Q - log2 3/8)) / (P + Q))."""
    x = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.float64)
    w = np.array([1, 1, 0, 0, 1, 1, 2, 2], dtype=np.float64) / 8
    res = orc.column(x, w)
    p, q = 0.5, 0.25
    want = math.sqrt((p * (math.log2(p) - math.log2(0.375)) + q * (math.log2(q) - math.log2(0.375))) / (p + q))
    d = float(orc.distance(res["js"], res["bound"])[0])
    assert abs(d - want) <= 4 * 2.0 ** -53 * want and abs(d - 0.285839405865445) < 1e-15
    assert res["bound"][0] == 0.75 and res["pint"][0] == 0.5 and res["qint"][0] == 0.25 and res["flag"] == 0
    # of -x the gap sits at P = 1/2, Q = 3/4
    p, q = 0.5, 0.75
    want_neg = math.sqrt((p * (math.log2(p) - math.log2(0.625)) + q * (math.log2(q) - math.log2(0.625))) / (p + q))
    assert abs(float(orc.distance(res["js_neg"], res["bound_neg"])[0]) - want_neg) <= 4 * 2.0 ** -53 * want_neg
    assert res["wmean"][0] == 0.75 and abs(res["wsd"][0] - math.sqrt(0.1875)) <= 2.0 ** -52


@pytest.mark.parametrize("n", cases.MP_SIZES)
def test_the_sums_against_50_digits(n):
    """|js - exact| <= (depth + 6) u A: the yardstick is sound (NumPy's log2 is within an ulp)."""
    import mpmath
    x, w = cases.values(n, 100 + n), cases.weights(3, n, 200 + n)
    order = np.argsort(x, kind="stable")
    for v in range(3):
        for s, q in ((x[order], w[v][order]), (-x[order][::-1], w[v][order][::-1])):
            got = orc.sums(s, q)
            js, bound = orc.sums_mp(s, q)
            allowed = (orc.depth(n) + 6) * orc.U * got["magnitude"]
            err = abs(mpmath.mpf(got["js"]) - js)
            print(f"[psens-mp] n={n} v={v}: |js - exact| / allowed = {float(err / allowed):.3g}")
            assert err <= allowed
            assert abs(mpmath.mpf(got["bound"]) - bound) <= (orc.depth(n) + 2) * orc.U * bound


def test_the_distance_does_not_see_a_power_of_two_scale():
    x, w = cases.values(257, 3), cases.weights(3, 257, 4)
    assert _bits(_d(x, w)) == _bits(_d(x * 4.0, w)) == _bits(_d(x * 2.0 ** -30, w))


def test_the_distance_under_a_shift_agrees_to_rounding():
    """x + c moves every gap by at most 2 u (|c| + max |x|), against gaps of the order of the range over N: 1e-9 relative
    leaves four digits to the few gaps that are much smaller, which carry as little of the sums."""
    x, w = cases.values(64, 7), cases.weights(3, 64, 8)
    assert np.allclose(_d(x + 1.0, w), _d(x, w), rtol=1e-9, atol=0)


def test_a_permutation_of_the_draws_changes_no_bit_without_ties():
    x, w = cases.values(1000, 11), cases.weights(3, 1000, 12)
    perm = np.random.default_rng(13).permutation(1000)
    a, b = orc.column(x, w), orc.column(x[perm], w[:, perm])
    for key in orc.OUTPUTS:
        assert _bits(a[key]) == _bits(b[key]), key


def test_equal_weights_give_exactly_zero():
    """q = 1: the prefix sums are integers, Q = P bit for bit, M = P, every log difference is 0."""
    x = cases.values(1000, 17)
    res = orc.column(x, np.full((1, 1000), 0.001), vflag=[orc.VFLAG_CONSTANT])
    assert res["js"][0] == 0.0 and res["js_neg"][0] == 0.0 and res["bound"][0] == 2.0 * res["pint"][0] > 0.0
    assert abs(res["wmean"][0] - x.mean()) <= 1e-15 and abs(res["wsd"][0] - x.std()) <= 1e-14
    # while the same weights pushed through the prefix sum leave a distance that is not zero (the square root amplifies rounding)
    plain = orc.column(x, np.full((1, 1000), 0.001))
    assert 0.0 <= float(orc.distance(plain["js"], plain["bound"])[0]) < 1e-6


def test_flags_of_constant_and_non_finite_columns():
    w = cases.weights(2, 8, 1)
    res = orc.column(np.full(8, 2.5), w)
    assert res["flag"] == orc.FLAG_CONSTANT and res["js"].tolist() == [0.0, 0.0] and res["bound"].tolist() == [0.0, 0.0]
    assert np.all(np.abs(res["wmean"] - 2.5) <= 2.0 ** -50) and np.all(res["wsd"] <= 2.0 ** -50)    # (a quotient of two rounded sums)
    bad = orc.column(np.array([0.0, 1.0, np.inf, 2.0]), w[:, :4])
    assert bad["flag"] == orc.FLAG_NONFINITE and all(np.isnan(bad[k]).all() for k in orc.OUTPUTS)
    assert orc.distance([0.0, 1.0, np.nan], [0.0, 4.0, 1.0]).tolist()[:2] == [0.0, 0.5]


def test_a_conjugate_normal_case_has_a_sensitivity_of_the_known_order():
    """x ~ N(0, 1) with the component log density -x^2 / 2: the power alpha scales the variance by 1 / alpha, and the CJS
    sensitivity of a scale change of that size is of the order of 0.1 (0.086 was seen when the unit was specified)."""
    x = cases.values(1000, 0)
    table = np.stack([x, -0.5 * x * x], axis=1)
    sens, rows, res, k, flags = orc.powerscale(table, [1], 0.01)
    print(f"[psens-conjugate] sensitivity {sens[0, 0]:.4f}, k {k.tolist()}")
    assert 0.03 < sens[0, 0] < 0.3 and not flags.any() and np.all(k < 0.7)
    assert np.all(rows >= 0.0) and res["flag"].tolist() == [0, 0]
    # the weighted sd moves the way the power says: alpha < 1 widens, alpha > 1 narrows, by about delta / 2
    assert res["wsd"][0, 0] > x.std() > res["wsd"][1, 0]
    assert abs(res["wsd"][1, 0] / res["wsd"][0, 0] - 1.0 / 1.01) < 2e-3


def test_psis_is_the_elpd_checkers_by_construction():
    r = cases.ratios(1000, 21, "normal") * 0.01
    lw, k, flag = orc.psis_weights(r)
    want, want_k = eorc.psis_column(-r)
    assert _bits(lw) == _bits(want) and k == want_k and flag == 0
    lw, k, flag = orc.psis_weights(np.full(25, -3.0))
    assert flag == orc.VFLAG_CONSTANT and k == np.inf and np.all(lw == -math.log(25))
    assert orc.scales(0.01) == (1.0 / 1.01 - 1.0, 1.01 - 1.0)
    x = np.stack([cases.values(25, 2), cases.ratios(25, 3, "heavy")], axis=1)
    lws, ks, ess, flags = orc.component_weights(x, [1], 0.5)
    assert lws.shape == (2, 25) and np.allclose(np.exp(lws).sum(axis=1), 1.0) and np.all((ess > 1.0) & (ess <= 25.0))
    assert _bits(lws[1]) == _bits(eorc.psis_column(-(0.5 * x[:, 1]))[0])


def test_stack_drops_the_burn_in_per_chain():
    a, b = np.arange(12.0).reshape(6, 2), np.arange(100.0, 110.0).reshape(5, 2)
    assert orc.stack([a, b], [2, 1])[:, 0].tolist() == [4.0, 6.0, 8.0, 10.0, 102.0, 104.0, 106.0, 108.0]
    assert np.array_equal(orc.sensitivity(np.array([[0.1], [0.3]]), 1.0), [[0.2]])
