"""Device against oracle and against a 50-digit evaluation for the Gibbs weights step (sbayes_amd/csrc/sbe_wgibbs.hip) where
tests/test_gpu_wgibbs.py does not reach: weights down to float32 denormals and exact zeros at every place of the row and every
C from 2 to 8, normalising sums of 0, a2 = 0 and 1 and denormal, A = 1 and B = 1 exactly, alpha from 1e-3 to 1e4, T from 1e-3
to 1e3, u = 0 and 1 - 2^-24, log_p NaN, +inf and -inf, uniforms one float32 step from p, object counts around the sweep, 64
patterns over two feature tiles, the last of three slots, features moved to other places of the table.  The cases are
tests/_wgibbs_range_cases.py; tests/test_wgibbs_range_cpu.py asserts under the oracle alone what each is there for, that no
decision lies within twice the band of its uniform and that the oracle lies within a quarter of the band of the 50-digit value.
The comparison is check_proposal's of tests/test_gpu_wgibbs.py (counts and w_new bit-equal, accept and the output rows equal,
NaN and infinite log_p equal, finite log_p within the band of the oracle) and |log_p_device - mp| <= band."""
import numpy as np
import pytest

from sbayes_amd import wgibbs
from tests import _wgibbs_range_cases as cases
from tests._wgibbs_range_cases import FINITE
from tests.test_gpu_wgibbs import bind, check_proposal, make_engine

pytestmark = pytest.mark.gpu


def _engine(c):
    eng = make_engine(c["na"], c["w"].shape[1], n_slots=c["n_slots"])
    bind(eng, c["slot"], c["has_components"], c["src"], c["w"])
    return eng


def _args(c):
    return c["i1"], c["i2"], c["a2"], c["u"], c["alpha"], c["beta_ab"], c["t"]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_against_the_oracle_and_the_50_digit_values(name):
    c = cases.case(name)
    fin = c["cls"] == FINITE
    assert (c["margin"][fin] > 2 * c["band"][fin]).all()                      # nothing is excluded (the generator's condition)
    with _engine(c) as eng:
        _counts, w_out, accept, log_p = check_proposal(eng, c["slot"], name, c["w"], c["has_components"], c["src"], c["na"], *_args(c))
    dist = cases.distance_to_mp(c, log_p)
    least = np.min(c["margin"][fin] / np.maximum(c["band"][fin], 1e-300), initial=np.inf)
    print(f"[wgibbs-range] {name}: worst |dev - mp| / band {np.max(dist[fin], initial=0.0):.3g}, least margin / band {least:.3g}, "
          f"classes finite/nan/+inf/-inf {'/'.join(map(str, cases.class_counts(cases.classes(log_p))))}")
    assert np.array_equal(cases.classes(log_p), c["cls"])
    assert (dist[fin] <= 1.0).all(), (name, np.flatnonzero(fin & ~(dist <= 1.0)).tolist())
    assert np.array_equal(accept, c["accept"]) and w_out.tobytes() == c["w_out"].tobytes()
    if "close" in c:                                                          # u one or two float32 steps from p
        assert np.array_equal(accept[c["close"]], np.full(c["close"].sum(), c["side"] != "above"))


def _run(c):
    """(pair_counts, w_out, accept, log_p) of one call on a fresh engine, and the same of a second call on it."""
    with _engine(c) as eng:
        return [[wgibbs.pair_counts(eng, c["slot"], c["i1"], c["i2"])] + list(wgibbs.step(eng, c["slot"], *_args(c))) for _ in range(2)]


def test_a_feature_has_the_same_bits_at_any_place_of_the_table():
    """The features permuted, and rotated by 5 (across the edge of the 16-feature tile): feature for feature the same bits of
    w_out, accept and log_p, and pair_counts permuted the same way."""
    c = cases.case(cases.PLACE_CASE)
    f = c["w"].shape[0]
    assert f > 16 + 5
    base, again = _run(c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
    for order in (np.random.default_rng(7).permutation(f), np.roll(np.arange(f), 5)):
        moved, _ = _run(cases.replaced(c, order))
        for k, (a, b) in enumerate(zip(moved, base)):
            assert a.dtype == b.dtype and a.tobytes() == b[order].tobytes(), (order.tolist(), k)


@pytest.mark.parametrize("name", ["B_T0.001", "C_n1541_c4_above", "D_p64_c8", "D_n4099", "D_slot2_of_3"])
def test_two_calls_on_the_same_state_return_the_same_bits(name):
    first, second = _run(cases.case(name))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
