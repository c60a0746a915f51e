"""GPU checks of the posterior predictive check (include/sbe_ppc.h, sbayes_amd/ppc.py) against the oracle (tests/_ppc_oracle.py).
The replicate, the counts and n_skipped must equal the oracle's in every case: the margin condition (asserted on the CPU for
every case that draws from Philox, tests/test_ppc_oracle_cpu.py) or exact dyadic arithmetic makes that a fair demand.  The
deviance sums lie within the band 2^-50 (n_terms + 4) sum |d| of the oracle's, +inf compared by class; the worst ratio to the
band is printed."""
import ctypes as ct
import math

import numpy as np
import pytest

from sbayes_amd import ppc
from sbayes_amd._handle import EngineError, _ptr
from tests import _ppc_cases as cases
from tests import _ppc_oracle as orc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_DATA = 1, 3, 4
NA = orc.NA


def _set(h, case):
    h.set_data(case["codes"], case["groups"], case["n_groups"], case["tables"].shape[3], case["clusters"].shape[1])


def _device(case, seed=0, uniforms=None, tile=0, splits=None):
    """The PpcResult of the device for a case, the samples split at `splits` (the handle continues the draw index)."""
    T = case["clusters"].shape[0]
    h = ppc.PpcHandle(0)
    try:
        _set(h, case)
        h.set_feature_tile(tile)
        edges = [0, *(splits or []), T]
        for a, b in zip(edges, edges[1:]):
            h.check(case["clusters"][a:b], case["weights"][a:b], case["tables"][a:b], seed=seed,
                    uniforms=None if uniforms is None else uniforms[a:b], replicates=True)
        return h.result()
    finally:
        h.close()


def _same_bits(a, b):
    return all(np.array_equal(getattr(a, k).view(np.uint8), getattr(b, k).view(np.uint8)) for k in ("y_rep", "dev_feature", "dev_object", "count_rep")) \
        and a.n_skipped == b.n_skipped and a.n_samples == b.n_samples


def _check(res, want, label=""):
    """The device's result against the oracle's check(); returns the worst deviance error in units of the band."""
    assert np.array_equal(res.y_rep, want["y_rep"]) and np.array_equal(res.count_rep, want["count_rep"]) and res.n_skipped == want["n_skipped"]
    d, drawn = want["d"], want["drawn"]
    worst = 0.0
    with np.errstate(invalid="ignore"):
        for got, ref, terms, total in ((res.dev_feature, want["dev_feature"], drawn.sum(axis=1)[:, None, :], np.abs(d).sum(axis=2)),
                                      (res.dev_object, want["dev_object"], drawn.sum(axis=2)[:, None, :], np.abs(d).sum(axis=3))):
            infinite = np.isinf(ref)
            assert np.array_equal(np.isinf(got), infinite) and not np.isnan(got).any() and (got[infinite] > 0).all()
            band = orc.dev_band(terms, np.where(infinite, 0.0, total))
            err = np.where(infinite, 0.0, np.abs(got - ref))
            assert (err <= band).all()
            worst = max(worst, float(np.max(np.where(band > 0, err / np.where(band > 0, band, 1.0), 0.0))))
    print(f"{label}: worst deviance error {worst:.3g} of the band "
          f"({'bit-identical' if np.array_equal(res.dev_feature, want['dev_feature']) and np.array_equal(res.dev_object, want['dev_object']) else 'differs'})")
    return worst


# ---- the recorded runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1])
def test_the_recorded_runs_match_the_oracle(r):
    case, want = cases.recorded(r), cases.recorded_oracle(r)
    res = _device(case, seed=cases.SEED)
    _check(res, want, f"run {r}")
    assert res.n_samples == 60 and res.n_skipped == 0 and res.kernel_ms > 0
    assert np.array_equal(res.p_feature, orc.p_value(want["dev_feature"][:, 1], want["dev_feature"][:, 0]))
    assert np.array_equal(res.p_object, orc.p_value(want["dev_object"][:, 1], want["dev_object"][:, 0]))
    total = want["dev_feature"].sum(axis=2)
    assert res.p_total == float(orc.p_value(total[:, 1], total[:, 0]))
    assert np.array_equal(res.p_count, orc.p_value(want["count_rep"], res.count_obs[None]))
    print(f"run {r}: p_feature {res.p_feature.min():.2f} to {res.p_feature.max():.2f}, median {np.median(res.p_feature):.2f}; "
          f"p_object {res.p_object.min():.2f} to {res.p_object.max():.2f}, median {np.median(res.p_object):.2f}; p_total {res.p_total:.3f}")


def test_the_one_call_form_discards_the_burn_in_and_keeps_the_draw_index_of_what_is_left():
    case = cases.recorded(0)
    res = ppc.posterior_predictive_check(case["codes"], case["groups"], case["clusters"], case["weights"], case["tables"], burnin=0.1, seed=cases.SEED,
                                         n_groups=case["n_groups"], replicates=True, device=0)
    kept = {k: (v[6:] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}
    _check(res, orc.check(seed=cases.SEED, **kept), "after burn-in")
    assert res.n_samples == 54 and res.y_rep.shape == (54, 100, 36)


# ---- seeded cases at the edges of the tile plan ----------------------------------------------------------------------------------
def _tiles_that_fit(case):
    R, S, C = case["tables"].shape[1], case["tables"].shape[3], case["weights"].shape[2]
    return [t for t in (1, 3, 16, 256) if 2 * t * (R * S + C) * 8 <= 160 << 10]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_seeded_cases_match_the_oracle_at_every_tile(shape):
    case, seed, want = cases.synthetic(shape)
    res = _device(case, seed=seed)
    _check(res, want, str(shape))
    tiles = _tiles_that_fit(case)
    assert 1 in tiles                                                         # (1 x 1 x 2 runs all four, R = 256 x S = 32 only this one)
    for tile in tiles:
        assert _same_bits(_device(case, seed=seed, tile=tile), res), tile


def test_the_largest_table_is_refused_at_two_features_per_tile():
    case, seed, _want = cases.synthetic(cases.SHAPES[-1])                     # R = 256 rows of S = 32 states
    h = ppc.PpcHandle(0)
    try:
        _set(h, case)
        h.set_feature_tile(2)
        with pytest.raises(EngineError, match="bytes of LDS") as err:
            h.check(case["clusters"], case["weights"], case["tables"], seed=seed)
        assert err.value.code == ERR_ARG and h.n_samples == 0
        with pytest.raises(EngineError, match="features=257 out of range") as err:
            h.set_feature_tile(257)
        assert err.value.code == ERR_ARG
    finally:
        h.close()


def test_the_split_of_the_samples_and_the_call_change_no_bit():
    shape = (33, 15, 2, 3, 3, None)
    case, seed, _ = cases.synthetic(shape, T=7)
    whole = _device(case, seed=seed)
    _check(whole, orc.check(seed=seed, **case), "T = 7")
    assert _same_bits(_device(case, seed=seed, splits=[1, 3]), whole)         # 1 + 2 + the rest, the draw index continued
    assert _same_bits(_device(case, seed=seed), whole)                        # the same call again
    other = _device(case, seed=seed + 1)
    assert not np.array_equal(other.y_rep, whole.y_rep) and np.array_equal(other.dev_feature[:, 0], whole.dev_feature[:, 0])


# ---- explicit uniforms --------------------------------------------------------------------------------------------------------------
def test_the_hand_case():
    case, uniforms, want = cases.hand()
    res = _device(case, uniforms=uniforms)
    assert res.y_rep.tolist() == want["y_rep"] and res.count_rep.tolist() == want["count_rep"] and res.n_skipped == 0
    _check(res, orc.check(uniforms=uniforms, **case), "hand")
    assert np.allclose(res.dev_feature, want["dev_feature"], rtol=2.0 ** -50, atol=0) and np.allclose(res.dev_object, want["dev_object"], rtol=2.0 ** -50, atol=0)
    assert res.p_feature.tolist() == [0.25] and res.p_object.tolist() == [0.5, 0.25]


def test_the_grid_draws_every_state_in_proportion():
    case, uniforms = cases.grid()
    for tile in (0, 1, 3):
        res = _device(case, uniforms=uniforms, tile=tile)
        assert res.count_rep.sum(axis=(0, 1)).tolist() == [256, 0, 512, 256]
        _check(res, orc.check(uniforms=uniforms, **case), f"grid, tile {tile}")


def test_uniforms_at_the_edges_of_the_draw_rule():
    """u = 0, u = 1 - 2^-53, u on and just below every cdf step of dyadic rows; zero-mass states first, in the middle and last;
    an observed state of zero mass; an object in no cluster and no group; an all-NA feature and an all-NA object."""
    case, uniforms, want_y = cases.edges()
    res = _device(case, uniforms=uniforms)
    assert res.y_rep[0].tolist() == want_y and res.n_skipped == 3
    _check(res, orc.check(uniforms=uniforms, **case), "edges")
    assert res.dev_feature[0, 0, 0] == math.inf and res.p_feature[0] == 0.0 and res.dev_object[0, 0, 0] == math.inf
    assert (res.dev_object[0, :, 4:6] == 0).all() and (res.dev_feature[0, :, 3] == 0).all() and res.p_object[5] == 0.5 and res.p_feature[3] == 0.5
    assert res.table("object")[1][5][5] == "no cells" and res.table("feature")[1][3][5] == "no cells"


def test_the_largest_uniform_draws_the_last_state_with_mass():
    """The clamp's neighbourhood: totals just above and just below 1 with trailing states of no mass.  v = u total never
    reaches total for a valid uniform (tests/test_ppc_oracle_cpu.py), so the count alone ends at the last state with mass;
    u = 1, where the clamp would act, is refused by the validation (below)."""
    case, uniforms = cases.off_one()
    res = _device(case, uniforms=uniforms)
    assert (res.y_rep == 1).all() and res.count_rep[0].tolist() == [[0, 2, 0, 0]] * 2
    _check(res, orc.check(uniforms=uniforms, **case), "off one")


# ---- validation ------------------------------------------------------------------------------------------------------------------
def _message(t, kind, at, F, S, C):
    return {0: f"sample {t}: object {at} is in more than one cluster",
            1: f"sample {t}: weights[{at // C}][{at % C}] is negative or not finite",
            2: f"sample {t}: the weights of feature {at} sum further than",
            3: f"sample {t}: tables[{at // S // F}][{at // S % F}][{at % S}] (row, feature, state) is negative or not finite",
            4: f"sample {t}: table row {at // F}, feature {at % F} has no positive entry",
            5: f"sample {t}: table row {at // F}, feature {at % F} sums further than",
            6: f"sample {t}: uniforms[{at}] (object {at // F}, feature {at % F}) is outside [0, 1) or not finite"}[kind]


def _raw_check(h, case, uniforms, first_draw=0):
    """sbe_ppc_check without the handle's own checks; returns (code, the outputs, which were filled with a sentinel)."""
    T, _K, N = case["clusters"].shape
    F, S = case["tables"].shape[2:]
    clusters, weights, tables = (np.ascontiguousarray(case[k]) for k in ("clusters", "weights", "tables"))
    y = np.full((T, N, F), 77, dtype=np.uint8)
    dev_f, dev_o = np.full((T, 2, F), -7.0), np.full((T, 2, N), -7.0)
    count = np.full((T, F, S), -7, dtype=np.int32)
    skipped = ct.c_int64(-7)
    u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float64)
    rc = h._lib.sbe_ppc_check(h._h, T, first_draw, 5, _ptr(clusters), _ptr(weights), _ptr(tables), _ptr(u) if u is not None else None, _ptr(y),
                              _ptr(dev_f), _ptr(dev_o), _ptr(count), ct.byref(skipped))
    return rc, (y, dev_f, dev_o, count, skipped.value)


def _untouched(outputs):
    y, dev_f, dev_o, count, skipped = outputs
    return (y == 77).all() and (dev_f == -7).all() and (dev_o == -7).all() and (count == -7).all() and skipped == -7


@pytest.mark.parametrize("kind", range(7), ids=orc.KINDS)
def test_every_kind_of_offender_is_named_and_nothing_is_written(kind):
    shape = (17, 16, 3, 2, 2, None)
    good, seed, _ = cases.synthetic(shape)
    case = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in good.items()}
    N, F, S, C = 17, 16, 3, 2
    uniforms = orc.uniforms_of(seed, 0, 3, N * F)
    uniforms[2, 5] = 1.0                                                      # a later sample's offender never wins
    if kind == 0:
        case["clusters"][1, :, 9] = 1
    elif kind == 1:
        case["weights"][1, 4, 1] = -0.25
    elif kind == 2:
        case["weights"][1, 4] = [0.5, 0.5001]
    elif kind == 3:
        case["tables"][1, 2, 7, 1] = math.nan
    elif kind == 4:
        case["tables"][1, 2, 7] = 0.0
    elif kind == 5:
        case["tables"][1, 2, 7] = [0.5, 0.25, 0.2]
    else:
        uniforms[1, 40], uniforms[1, 200] = -0.5, math.inf
    if kind < 6:
        uniforms[1, 3] = 2.0                                                  # the same sample's uniform comes after every other kind
        case["tables"][1, 2, 9, 0] += 0.5 if kind < 5 else 0.0                # ... and so does a later kind (a table sum) after this one
    t, found, at = orc.first_offender(case["clusters"], case["weights"], case["tables"], uniforms)
    assert (t, found) == (1, kind)
    h = ppc.PpcHandle(0)
    try:
        _set(h, case)
        rc, outputs = _raw_check(h, case, uniforms)
        assert rc == ERR_DATA and _message(t, found, at, F, S, C) in h._last_error() and _untouched(outputs)
        rc, outputs = _raw_check(h, good, None)                               # the handle stays usable
        assert rc == 0 and not _untouched(outputs) and np.array_equal(outputs[0], _device(good, seed=5).y_rep)
    finally:
        h.close()


def test_state_and_staging_errors():
    case, _seed, _ = cases.synthetic((17, 16, 3, 2, 2, None))
    h = ppc.PpcHandle(0)
    try:
        rc, outputs = _raw_check(h, case, None)
        assert rc == ERR_STATE and "no data yet (sbe_ppc_set_data comes first)" in h._last_error() and _untouched(outputs)
        _set(h, case)
        one = h.max_samples(replicates=True)
        dummy = np.zeros(8)
        past = h._lib.sbe_ppc_check(h._h, one + 1, 0, 0, _ptr(dummy), _ptr(dummy), _ptr(dummy), None, _ptr(dummy), None, None, None, None)
        assert past == ERR_ARG and f"at most {one} samples per call here" in h._last_error()
        assert h._lib.sbe_ppc_check(h._h, -1, 0, 0, _ptr(dummy), _ptr(dummy), _ptr(dummy), None, None, None, None, None, None) == ERR_ARG
        assert h._lib.sbe_ppc_check(h._h, 1, -1, 0, _ptr(dummy), _ptr(dummy), _ptr(dummy), None, None, None, None, None, None) == ERR_ARG
        assert "first_draw=-1 is negative" in h._last_error()
        assert h._lib.sbe_ppc_check(h._h, 1, 0, 0, None, _ptr(dummy), _ptr(dummy), None, None, None, None, None, None) == ERR_ARG
        assert "null pointer argument: clusters" in h._last_error()
        skipped = ct.c_int64(-7)
        assert h._lib.sbe_ppc_check(h._h, 0, 0, 0, None, None, None, None, None, None, None, None, ct.byref(skipped)) == 0 and skipped.value == 0
        # every output is optional: the same call with only the counts asked for gives the same counts
        rc, outputs = _raw_check(h, case, None)
        clusters, weights, tables = (np.ascontiguousarray(case[k]) for k in ("clusters", "weights", "tables"))
        count = np.zeros_like(outputs[3])
        assert h._lib.sbe_ppc_check(h._h, 3, 0, 5, _ptr(clusters), _ptr(weights), _ptr(tables), None, None, None, None, _ptr(count), None) == 0
        assert rc == 0 and np.array_equal(count, outputs[3])
    finally:
        h.close()
