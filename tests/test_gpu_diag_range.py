"""Device against checker for the column kernel (sbayes_amd/csrc/sbe_diag_column.hip.h) where tests/test_gpu_diag.py does not
reach: rho_t entries past the 2048 kept in LDS (the per-column global scratch, its allocation edge, its reuse across launches,
the monotone pass and the sums reading both memories, max_lag on the boundary), walks and stops on either side of the blocks
of 32 lags, locations to 1e9 and scales from 1e-120 to 1e120, the absolute constant threshold; the block-edge and magnitude
columns through the summary too (the derived store's addressing).  The cases are tests/_diag_range_cases.py;
tests/test_diag_range_cpu.py asserts under the checker alone what each is there for and that its decisions are safe.  The
comparison is that of tests/test_gpu_diag.py: n_lags and flag equal, every float output within the derived bound."""
import numpy as np
import pytest

from tests import _diag_range_cases as cases
from tests.test_gpu_diag import OUTPUTS, _check, _same_bits
from tests.test_gpu_summary import _bits
from tests.test_gpu_summary import _check as _summary_check
from tests.test_gpu_summary import _diag_equal
from sbayes_amd import diag, summary

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_matches_the_checker_within_the_derived_bounds(name):
    x, kw, want = cases.case(name)
    assert cases.safe(want).all()
    res = diag.convergence(list(x), **kw)
    _check(res, want, name)
    if name == "spill_global_8x2300":
        assert res.path == "global" and res.n_chains * res.n_draws == 18400 > diag.lds_max_draws()
    elif name.startswith(("alloc_", "spill_")):
        assert res.path == "lds"


def _compute(h, x, launch, **kw):
    m, s, p = x.shape
    h.set_launch_columns(launch)
    h.reset(m, p, s)
    for c in range(m):
        h.append(c, x[c])
    return h.compute(**kw)


def test_spilled_bits_do_not_depend_on_the_launch_size_or_the_column_position():
    """The scratch slice of a column is that of its workgroup: with 1 or 2 columns per launch the same column runs in another
    slice, and the scratch is used again by the next launch.  Column 0 again as the last column: the same bits in a fourth."""
    x, kw, want = cases.case("spill_2x2400")
    ref = diag.convergence(list(x), **kw)
    _check(ref, want, "spill_2x2400 (reference of the launch sizes)")
    wide = np.concatenate([x, x[:, :, :1]], axis=2)
    h = diag.DiagHandle()
    try:
        for launch, launches in ((0, 1), (1, 3), (2, 2)):
            res = _compute(h, x, launch, **kw)
            assert _same_bits(res, ref), launch
            assert res.launches == launches
        for launch in (0, 3):
            res = _compute(h, wide, launch, **kw)
            for k in OUTPUTS:
                v = getattr(res, k)
                assert v[:3].tobytes() == getattr(ref, k).tobytes() and v[3:].tobytes() == v[:1].tobytes(), (launch, k)
    finally:
        h.close()


def test_a_max_lag_above_the_walk_changes_no_bit():
    x, kw, _want = cases.case("edge_max_lag_398")
    ref = diag.convergence(list(x), burnin=0.0, split=False)
    assert ref.n_lags.tolist() == [397] and ref.flag.tolist() == [0]
    for k in cases.FREE_MAX_LAGS:
        assert _same_bits(diag.convergence(list(x), **cases.case(f"edge_max_lag_{k}")[1]), ref), k


def test_a_magnitude_column_has_the_same_bits_next_to_its_neighbours():
    x, kw, _want = cases.case("magnitudes")
    table = diag.convergence(list(x), **kw)
    for j, name in enumerate(cases.MAGNITUDES):
        one = diag.convergence(list(cases.case(name)[0]), **cases.case(name)[1])
        for k in OUTPUTS:
            assert getattr(table, k)[j:j + 1].tobytes() == getattr(one, k).tobytes(), (name, k)


# ---- the same columns through the summary: the derived store has cap = n and its own offsets -----------------------------------
@pytest.mark.parametrize("name", cases.SUMMARY_CASES)
def test_summary_of_the_block_edge_and_magnitude_columns(name):
    """Quantiles and HDI bit-equal, the five shared outputs bit-equal to the diagnostics', the rank outputs within bounds."""
    x, kw, want = cases.summary_case(name)
    assert want["margin_ok"].all()
    res = summary.summarize(list(x), **kw)
    _summary_check(res, want, f"{name} (range)")
    _diag_equal(res, x, kw)


def test_the_rank_outputs_do_not_depend_on_the_scale():
    """Scaling by 1e-7 keeps the order and the ties (asserted on the CPU), so the derived columns are the same bits and so are
    the outputs that come from them alone."""
    small, unit = (summary.summarize(list(cases.case(name)[0]), **cases.case(name)[1]) for name in ("scale_1e-7", "unit"))
    for k in ("rhat_rank", "ess_bulk", "ess_tail"):
        assert _bits(getattr(small, k)) == _bits(getattr(unit, k)), k
    assert _bits(small.sd) != _bits(unit.sd)
