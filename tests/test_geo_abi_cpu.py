"""CPU checks of the geo-prior boundary (include/sbe_geo.h, sbayes_amd/geo.py): the symbols are exported and bound by the
module's own prototype table, the limits agree, and bad arguments are refused before the device is touched."""
import ctypes as ct
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from sbayes_amd import geo
from tests import _abi_header as abi

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "sbe_geo.h").read_text()


def test_every_symbol_of_the_header_is_exported_and_bound():
    abi.check_symbols(geo, HEADER, 12)


def test_limits_and_codes_agree_with_the_header():
    assert abi.macro(HEADER, "SBE_GEO_MAX_OBJECTS") == str(geo.MAX_OBJECTS)
    assert abi.macro(HEADER, "SBE_GEO_MAX_MASKS") == "(1 << 20)" and geo.MAX_MASKS == 1 << 20
    assert abi.macro(HEADER, "SBE_GEO_MAX_LAUNCH_MASKS") == "(1 << 16)" and geo.MAX_LAUNCH_MASKS == 1 << 16
    assert abi.macro(HEADER, "SBE_GEO_LDS_MEMBERS") == str(geo.LDS_MEMBERS)
    assert geo.MAX_OBJECTS ** 2 * 8 == 8 << 30             # the cost matrix at the limit: 8 GiB, as SBE_EM_MAX_COST_BYTES
    assert (geo.LDS_MEMBERS ** 2 + geo.LDS_MEMBERS) * 8 + 8192 <= 160 * 1024       # the staged sub-matrix fits a workgroup's LDS
    for table, prefix in ((geo.SKELETONS, "SBE_GEO_SKELETON_"), (geo.AGGREGATIONS, "SBE_GEO_AGG_"), (geo.PROBABILITY_FUNCTIONS, "SBE_GEO_PROB_")):
        for name, code in table.items():
            assert abi.macro(HEADER, prefix + {"complete_graph": "COMPLETE"}.get(name, name.upper())) == str(code)


def test_every_array_handed_to_the_library_is_bound_to_a_name():
    abi.check_ptr_arguments(geo)


class _NoDevice(geo.GeoHandle):
    """A handle that holds a cost matrix of N objects as far as the host-side checks know; any library call fails the test."""
    def __init__(self, n):
        self.n_objects = n
        self._h = ct.c_void_p()

        def refuse(*a, **k):
            raise AssertionError("the device was touched")
        self._lib = SimpleNamespace(**{name: refuse for name in geo.PROTOTYPES})


@pytest.mark.parametrize("call,err,match", [
    (lambda h: h.prior(np.zeros((2, 9), dtype=bool), 1.0), ValueError, "must end in N = 10"),
    (lambda h: h.prior(np.zeros((2, 10), dtype=bool), 1.0), ValueError, "mask 0 has no member"),
    (lambda h: h.prior(np.ones((2, 10)), 1.0), TypeError, "bool"),
    (lambda h: h.prior(np.ones((2, 10), dtype=bool), 0.0), ValueError, "positive and finite"),
    (lambda h: h.prior(np.ones((2, 10), dtype=bool), 1.0, aggregation="median"), ValueError, "aggregation must be one of"),
    (lambda h: h.prior(np.ones((2, 10), dtype=bool), 1.0, probability_function="sigmoid"), ValueError, "inflection_point"),
    (lambda h: h.prior(np.ones((2, 10), dtype=bool), 1.0, skeleton="delaunay"), ValueError, "skeleton must be one of"),
    (lambda h: h.skeleton_costs(np.ones((2, 10), dtype=bool), skeleton="diameter"), ValueError, "skeleton must be one of"),
    (lambda h: h.costs_per_object(np.ones((2, 10), dtype=bool), 1.0), ValueError, "one mask"),
    (lambda h: h.costs_per_object(np.zeros(10, dtype=bool), 1.0), ValueError, "no member"),
    (lambda h: h.set_cost(np.zeros((3, 4))), ValueError, "square"),
    (lambda h: h.set_cost(np.broadcast_to(np.zeros((1, 1)), (geo.MAX_OBJECTS + 1,) * 2)), ValueError, "32768"),
])
def test_bad_input_is_refused_before_the_device(call, err, match):
    with pytest.raises(err, match=match):
        call(_NoDevice(10))


def test_too_many_masks_are_refused_with_the_limit():
    masks = np.broadcast_to(np.ones((1, 1), dtype=bool), (geo.MAX_MASKS + 1, 1))
    with pytest.raises(ValueError, match=r"2\^20"):
        _NoDevice(1).prior(masks, 1.0)


def test_c_abi_validates_before_the_device():
    assert sorted(abi.check_null_handles(geo)) == sorted(set(geo.PROTOTYPES) - {"sbe_geo_abi_version", "sbe_geo_last_error"})


def test_handles_are_not_picklable_and_enums_pass_as_strings():
    abi.check_not_picklable(geo.GeoHandle)
    import enum

    class Agg(str, enum.Enum):
        MEAN = "mean"
    assert geo._choice(Agg.MEAN, geo.AGGREGATIONS, "aggregation") == ("mean", 0)
    costs = geo.SkeletonCosts(*(np.array([v]) for v in (3, 2, 5.0, 4.0, 2.5)))
    assert costs.aggregate("mean") == 2.5 and costs.aggregate("sum") == 5.0 and costs.aggregate("max") == 4.0


def test_covered_says_which_priors_the_device_form_takes():
    def prior(**kw):
        base = dict(prior_type="cost_based", cost_matrix=np.zeros((2, 2)), aggregation_policy="mean", probability_function="exponential",
                    inflection_point=None, config=SimpleNamespace(skeleton="mst"))
        base.update(kw)
        return SimpleNamespace(**base)
    assert geo.covered(prior()) and geo.covered(prior(config=SimpleNamespace(skeleton="complete_graph")))
    assert not geo.covered(prior(config=SimpleNamespace(skeleton="delaunay")))
    assert geo.covered(prior(config=SimpleNamespace(skeleton="delaunay")), for_call=False)     # (the per-object form takes the MST anyway)
    assert not geo.covered(prior(prior_type="simulated")) and not geo.covered(prior(prior_type="uniform"))
    assert not geo.covered(prior(probability_function="sigmoid")) and geo.covered(prior(probability_function="sigmoid", inflection_point=3.0))
    assert not geo.covered(prior(cost_matrix=None)) and not geo.covered(SimpleNamespace())
