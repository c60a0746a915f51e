"""GPU checks of the per-cluster evidence unit (include/sbe_contrib.h, sbayes_amd/contribution.py) against the oracle
(tests/_contrib_oracle.py).  The m's of the device and of the oracle are bit-identical, so only the logs differ: both sums lie
within the band 2^-50 (n_terms + 4) sum (|log m_k| + |log m0|) of the oracle's, +inf compared by class, and n_skipped is equal.
The worst ratio to the band is printed (DESIGN.md section 24 records what the MI355X gave)."""
import ctypes as ct
import itertools
import math

import numpy as np
import pytest

from sbayes_amd import contribution, predict
from sbayes_amd._handle import EngineError, _ptr
from tests import _contrib_cases as cases
from tests import _contrib_oracle as orc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
NA = orc.NA
LDS = 160 << 10


def _set(h, case):
    h.set_data(case["codes"], case["groups"], case["n_groups"], case["tables"].shape[3], case["clusters"].shape[1])


def _run(h, case, tile=0, splits=()):
    """The result of handle `h`, which has the case's data, for the case's samples split at `splits`."""
    T = case["clusters"].shape[0]
    h.reset()
    h.set_feature_tile(tile)
    edges = [0, *splits, T]
    for a, b in zip(edges, edges[1:]):
        h.evaluate(case["clusters"][a:b], case["weights"][a:b], case["tables"][a:b])
    return h.result()


def _device(case, tile=0, splits=()):
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        return _run(h, case, tile, splits)
    finally:
        h.close()


def _same_bits(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)) for k in ("affinity", "gain_feature", "member")) \
        and a.n_skipped == b.n_skipped and a.n_samples == b.n_samples


def _check(res, want, label=""):
    """The device's result against the oracle's evaluate(); returns the worst error in units of the band."""
    assert res.n_skipped == want["n_skipped"] and np.array_equal(res.member, want["member"])
    (aff_terms, aff_mag), (gain_terms, gain_mag) = orc.terms_and_magnitudes(want)
    worst = 0.0
    with np.errstate(invalid="ignore"):
        for got, ref, terms, mag in ((res.affinity, want["affinity"], aff_terms, aff_mag), (res.gain_feature, want["gain_feature"], gain_terms, gain_mag)):
            infinite = np.isinf(ref)
            assert np.array_equal(np.isinf(got), infinite) and not np.isnan(got).any() and (got[infinite] > 0).all()
            band = orc.band(terms, np.where(infinite, 0.0, mag))
            err = np.where(infinite, 0.0, np.abs(got - ref))
            ratio = np.where(band > 0, err / np.where(band > 0, band, 1.0), 0.0)
            print(f"{label}: {got.shape} worst error {float(ratio.max()):.3g} of the band")
            assert (err <= band).all()
            worst = max(worst, float(ratio.max()))
    same = np.array_equal(res.affinity, want["affinity"]) and np.array_equal(res.gain_feature, want["gain_feature"])
    print(f"{label}: worst error {worst:.3g} of the band ({'bit-identical' if same else 'differs'})")
    return worst


# ---- the recorded runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1])
def test_the_recorded_runs_match_the_oracle(r):
    case, want = cases.recorded(r), cases.recorded_oracle(r)
    res = _device(case)
    _check(res, want, f"run {r}")
    assert res.n_samples == 60 and res.n_skipped == 0 and res.kernel_ms > 0
    assert res.rank() == orc.rank(res.gain_feature) and sorted(res.rank()) == [0, 1, 2]
    gain = res.gain
    print(f"run {r}: rank {res.rank()}, mean gain {gain.mean(axis=0).tolist()}")


def test_the_one_call_form_discards_the_burn_in():
    case = cases.recorded(0)
    res = contribution.cluster_contribution(case["codes"], case["groups"], case["clusters"], case["weights"], case["tables"], burnin=0.1,
                                            n_groups=case["n_groups"], device=0)
    whole = cases.recorded_oracle(0)
    kept = {k: (v[6:] if isinstance(v, np.ndarray) else v) for k, v in whole.items()}
    kept["n_skipped"] = 0
    _check(res, kept, "after burn-in")
    assert res.n_samples == 54 and res.affinity.shape == (54, 3, 100)


# ---- seeded cases: the smallest shapes at which each mechanism can go wrong ---------------------------------------------------------
def _fits(case, tile):
    R, S, C = case["tables"].shape[1], case["tables"].shape[3], case["weights"].shape[2]
    return 2 * tile * (R * S + C) * 8 <= LDS


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_seeded_cases_match_the_oracle_at_several_tiles(shape):
    case, want = cases.synthetic(shape)
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        res = _run(h, case)
        _check(res, want, str(shape))
        tiles = [t for t in (1, 2, 3, 5, 16, 19, 64, 256) if _fits(case, t)]
        assert tiles[:4] == [1, 2, 3, 5]
        for tile in tiles:
            assert _same_bits(_run(h, case, tile), res), tile
    finally:
        h.close()
    if shape[3] == 1:                                                         # C = 1: every cell is skipped, the outputs are +0.0
        T, K = case["clusters"].shape[:2]
        assert res.n_skipped == T * K * int((case["codes"] != NA).sum())
        for out in (res.affinity, res.gain_feature):
            assert (out == 0.0).all() and not np.signbit(out).any()


def test_every_feature_tile_that_fits_gives_the_same_bits():
    case, want = cases.synthetic((17, 7, 5, 3, 3, None))
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        res = _run(h, case)
        _check(res, want, "default tile")
        tiles = [t for t in range(1, 257) if _fits(case, t)]                 # (at most 9 rows of 5 states: more than half of them fit)
        assert len(tiles) >= 128
        for tile in tiles:
            assert _same_bits(_run(h, case, tile), res), tile
    finally:
        h.close()


def test_any_split_of_the_samples_and_the_call_change_no_bit():
    shape = (17, 7, 5, 3, 3, None)
    T = 5
    case, want = cases.synthetic(shape, T=T)
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        whole = _run(h, case)
        _check(whole, want, "T = 5")
        assert _same_bits(_run(h, case), whole)                               # the same call again
        for r in range(1, T):
            for splits in itertools.combinations(range(1, T), r):           # every composition of the five samples
                assert _same_bits(_run(h, case, splits=splits), whole), splits
    finally:
        h.close()
    assert _same_bits(_device(case), whole)                                   # and from another handle


# ---- cases by construction ------------------------------------------------------------------------------------------------------------
def test_the_dyadic_hand_case_is_bit_exact():
    case, want = cases.hand()
    res = _device(case)
    assert res.affinity.tolist() == want["affinity"] and res.gain_feature.tolist() == want["gain_feature"]
    assert not np.signbit(res.affinity[:, 0, 1]).any() and not np.signbit(res.gain_feature[:, :, 1]).any()   # d = +0.0 exactly
    assert res.n_skipped == 0 and res.rank() == want["rank"]
    assert _check(res, orc.evaluate(**case), "hand") == 0.0


def test_a_members_row_is_the_posterior_predictives():
    """T = 1, F = 1, so affinity[0, k, n] is the one d of the object.  predict's lik entry of a member of k is float32(m_k) and of an
    object in no cluster float32(m0), bit for bit; through exp of the device's d, m_k is read back only within the band."""
    case = orc.predict_orc.random_case(2431, 40, 1, 4, 3, 2, 1, na_share=0.0)
    want = orc.evaluate(**case)
    res = _device(case)
    _check(res, want, "F = 1")
    lik = predict.posterior_predictive(case["codes"], case["groups"], case["clusters"], case["weights"], case["tables"], burnin=0.0, lik=True, device=0,
                                       n_groups=case["n_groups"]).lik[0]
    ids, _ = orc.cluster_ids(case["clusters"][0])
    checked = 0
    for n in range(40):
        if not want["counted"][0, :, n, 0].all():
            continue
        m0 = want["m0"][0, n, 0]
        if ids[n] < 0:
            assert lik[n] == np.float32(m0)
            continue
        k = ids[n]
        mk = want["m"][0, k, n, 0]
        assert lik[n] == np.float32(mk)
        band = orc.band(1, abs(math.log(mk)) + abs(math.log(m0)))
        # the device's d is within the band of the oracle's, which is within a quarter of it of log(m_k / m0); exp, the product
        # and the quotient round once each
        assert abs(math.exp(res.affinity[0, k, n]) * m0 / mk - 1.0) <= math.expm1(1.25 * band) + 2.0 ** -51
        checked += 1
    assert checked >= 10


def test_no_mass_outside_the_cluster_is_plus_infinity_in_both_sums():
    case, want = cases.no_mass_outside()
    res = _device(case)
    assert res.affinity.tolist() == want["affinity"] and res.gain_feature.tolist() == want["gain_feature"] and res.n_skipped == want["n_skipped"]
    _check(res, orc.evaluate(**case), "m0 = 0")


def test_exactly_the_cells_of_an_object_without_a_group_are_skipped():
    case = cases.without_a_group()
    want = orc.evaluate(**case)
    res = _device(case)
    _check(res, want, "without a group")
    T, K, _N = case["clusters"].shape
    assert res.n_skipped == T * K * int((case["codes"][[1, 3]] != NA).sum()) > 0
    assert (res.affinity[:, :, [1, 3]] == 0.0).all() and not np.signbit(res.affinity[:, :, [1, 3]]).any() and (res.affinity[:, :, [0, 2]] != 0.0).all()


# ---- validation ------------------------------------------------------------------------------------------------------------------
def _message(t, kind, at, F, S, C):
    return {0: f"sample {t}: object {at} is in more than one cluster",
            1: f"sample {t}: weights[{at // C}][{at % C}] is negative or not finite",
            2: f"sample {t}: the weights of feature {at} sum further than",
            3: f"sample {t}: tables[{at // S // F}][{at // S % F}][{at % S}] (row, feature, state) is negative or not finite",
            4: f"sample {t}: table row {at // F}, feature {at % F} has no positive entry",
            5: f"sample {t}: table row {at // F}, feature {at % F} sums further than"}[kind]


def _raw(h, case):
    """sbe_contrib_evaluate without the handle's own checks; returns (code, the outputs, which were filled with a sentinel)."""
    T, K, N = case["clusters"].shape
    F = case["tables"].shape[2]
    clusters, weights, tables = (np.ascontiguousarray(case[k]) for k in ("clusters", "weights", "tables"))
    affinity, gain = np.full((T, K, N), -7.0), np.full((T, K, F), -7.0)
    skipped = ct.c_int64(-7)
    rc = h._lib.sbe_contrib_evaluate(h._h, T, _ptr(clusters), _ptr(weights), _ptr(tables), _ptr(affinity), _ptr(gain), ct.byref(skipped))
    return rc, (affinity, gain, skipped.value)


def _untouched(outputs):
    affinity, gain, skipped = outputs
    return (affinity == -7).all() and (gain == -7).all() and skipped == -7


@pytest.mark.parametrize("kind", range(6), ids=orc.KINDS)
def test_every_kind_of_offender_is_named_and_nothing_is_written(kind):
    shape = (17, 7, 5, 3, 3, None)
    good, want = cases.synthetic(shape)
    case = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in good.items()}
    F, S, C = 7, 5, 3
    case["weights"][2, 1, 0] = -1.0                                           # a later sample's offender never wins
    if kind == 0:
        case["clusters"][1, :, 9] = 1
    elif kind == 1:
        case["weights"][1, 4, 1] = -0.25
    elif kind == 2:
        case["weights"][1, 4] = [0.5, 0.25, 0.2501]
    elif kind == 3:
        case["tables"][1, 2, 6, 1] = math.nan
    elif kind == 4:
        case["tables"][1, 2, 6] = 0.0
    else:
        case["tables"][1, 2, 6] = [0.5, 0.25, 0.2, 0.0, 0.0]
    if kind < 5:
        case["tables"][1, 4, 3] = [0.5, 0.5, 0.5, 0.0, 0.0]                   # the same sample's later kind (a table sum) comes after this one
    t, found, at = orc.predict_orc.first_offender(case["clusters"], case["weights"], case["tables"])
    assert (t, found) == (1, kind)
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        rc, outputs = _raw(h, case)
        assert rc == ERR_DATA and _message(t, found, at, F, S, C) in h._last_error() and _untouched(outputs)
        rc, outputs = _raw(h, good)                                           # the handle stays usable
        assert rc == 0 and np.array_equal(outputs[0], _device(good).affinity) and outputs[2] == want["n_skipped"]
    finally:
        h.close()


def test_state_and_staging_errors():
    case, want = cases.synthetic((17, 7, 5, 3, 3, None))
    h = contribution.ContributionHandle(0)
    try:
        rc, outputs = _raw(h, case)
        assert rc == ERR_STATE and "no data yet (sbe_contrib_set_data comes first)" in h._last_error() and _untouched(outputs)
        _set(h, case)
        one = h.max_samples()
        dummy = np.zeros(8)
        past = h._lib.sbe_contrib_evaluate(h._h, one + 1, _ptr(dummy), _ptr(dummy), _ptr(dummy), _ptr(dummy), None, None)
        assert past == ERR_ARG and f"at most {one} samples per call here" in h._last_error()
        assert h._lib.sbe_contrib_evaluate(h._h, -1, _ptr(dummy), _ptr(dummy), _ptr(dummy), None, None, None) == ERR_ARG
        assert h._lib.sbe_contrib_evaluate(h._h, 1, None, _ptr(dummy), _ptr(dummy), None, None, None) == ERR_ARG
        assert "null pointer argument: clusters" in h._last_error()
        skipped = ct.c_int64(-7)
        assert h._lib.sbe_contrib_evaluate(h._h, 0, None, None, None, None, None, ct.byref(skipped)) == 0 and skipped.value == 0
        # every output is optional: each alone gives the same bits, and none at all still counts what is skipped
        rc, (affinity, gain, n_skipped) = _raw(h, case)
        assert rc == 0 and n_skipped == want["n_skipped"]
        clusters, weights, tables = (np.ascontiguousarray(case[k]) for k in ("clusters", "weights", "tables"))
        alone = np.zeros_like(affinity)
        assert h._lib.sbe_contrib_evaluate(h._h, 3, _ptr(clusters), _ptr(weights), _ptr(tables), _ptr(alone), None, None) == 0
        assert np.array_equal(alone.view(np.uint8), affinity.view(np.uint8))
        alone = np.zeros_like(gain)
        assert h._lib.sbe_contrib_evaluate(h._h, 3, _ptr(clusters), _ptr(weights), _ptr(tables), None, _ptr(alone), None) == 0
        assert np.array_equal(alone.view(np.uint8), gain.view(np.uint8))
        assert h._lib.sbe_contrib_evaluate(h._h, 3, _ptr(clusters), _ptr(weights), _ptr(tables), None, None, ct.byref(skipped)) == 0
        assert skipped.value == want["n_skipped"]
        with pytest.raises(EngineError, match="features=257 out of range") as err:
            h.set_feature_tile(257)
        assert err.value.code == ERR_ARG
    finally:
        h.close()


def test_the_largest_table_is_refused_at_a_tile_that_does_not_fit_the_lds():
    case, _want = cases.synthetic((6, 2, 2, 2, 255, (1,)))                    # R = 256 rows of S = 2 states: 19 features fit
    assert case["tables"].shape[1] == 256 and _fits(case, 19) and not _fits(case, 20)
    h = contribution.ContributionHandle(0)
    try:
        _set(h, case)
        h.set_feature_tile(20)                                                # accepted here, refused at the next call
        with pytest.raises(EngineError, match="a tile of 20 features takes two slices of 256 rows x 2 states") as err:
            h.evaluate(case["clusters"], case["weights"], case["tables"])
        assert err.value.code == ERR_ARG and h.n_samples == 0
    finally:
        h.close()
