"""The collapsed likelihood's per-feature term on the device, entry by entry against a 40-digit evaluation and form against
form (the cases, the reference and the derived bound: tests/_collapsed_range_cases.py; tests/test_collapsed_range_cpu.py
asserts without a device that the checker is right and sharp).  The term's routines (sbe_dirichlet.hip.h) have three callers
-- k_dcl (<float> behind sbe_dirichlet_logpdf, <int32_t> behind the resident calls of a wide table), collapsed_group_block
(k_collapsed_groups, k_collapsed_source_prior) and the tile blocks of step_core_body -- each with its own thread mapping, its
own sums and (k_dcl: in place, the others: k_conc_lgamma's tables) its own source of lgamma(a); they must agree to the bit:

    1  Engine.dirichlet_logpdf, concentration shared and per group: every entry within the bound, +0.0 where E is exactly
       0, float32(E) on every sharp entry away from a midpoint;
    2  set_concentration + set_counts + collapsed_loglik(per_feature=True) (one launch, or the k_dcl / k_group_sum_f32 pair
       at F = 49, S = 254; component 1 with g_lo != 0): the same, and bit-equal to (1);
    3  collapsed_loglik, collapsed_loglik_all, collapsed_and_source_prior: per group NumPy's float32 sum of (2)'s rows, bit for bit;
    4  step() at the range's concentrations: the candidate's per-group values bit-equal to the stateless call on its counts."""
import numpy as np
import pytest

from sbayes_amd.engine import Engine
from tests import _collapsed_range_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_stateless_call_meets_the_bound_entry_by_entry(name):
    c = cases.case(name)
    with Engine(c.features, c.n_groups, n_slots=1) as eng:
        for comp in range(2):
            pf, pg = eng.dirichlet_logpdf(c.counts[comp], c.conc[comp], per_group=True)
            r = cases.assert_meets(cases.reference(name, comp), pf, (name, comp, "dirichlet_logpdf"))
            print(cases.line(f"{name} component {comp} dirichlet_logpdf", r))
            assert np.array_equal(pg, cases.group_sums(pf))
        # the shared table handed over once per group is the per-group form of the same pointer arithmetic
        spread = np.ascontiguousarray(np.broadcast_to(c.conc[0], c.counts[0].shape))
        assert eng.dirichlet_logpdf(c.counts[0], spread).tobytes() == eng.dirichlet_logpdf(c.counts[0], c.conc[0]).tobytes()


def _resident(c):
    """An engine with the case's concentrations and counts in slot 0, and what collapsed_and_source_prior asks for beside
    them: every object in a group of both components, every source the first component."""
    eng = Engine(c.features, c.n_groups, n_slots=1)
    n = c.features.shape[0]
    src = np.zeros((n, c.F, 2), dtype=bool)
    src[..., 0] = True
    for comp in range(2):
        eng.set_concentration(comp, c.conc[comp])
        eng.set_groups(0, comp, np.arange(c.n_groups[comp])[:, None] == np.arange(n)[None, :] % c.n_groups[comp])
    eng.set_source(0, src)
    eng.set_weights(0, np.full((c.F, 2), 0.5, dtype=np.float32))
    for comp in range(2):
        eng.set_counts(0, comp, c.counts[comp])
    return eng


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_resident_calls_meet_the_bound_and_equal_the_stateless_call_bit_for_bit(name):
    c = cases.case(name)
    with _resident(c) as eng:
        sums = []
        for comp in range(2):
            assert np.array_equal(eng.get_counts(0, comp), c.counts[comp])
            pg, pf = eng.collapsed_loglik(0, comp, per_feature=True)
            r = cases.assert_meets(cases.reference(name, comp), pf, (name, comp, "collapsed_loglik"))
            print(cases.line(f"{name} component {comp} collapsed_loglik", r))
            stateless = eng.dirichlet_logpdf(c.counts[comp], c.conc[comp])
            assert pf.tobytes() == stateless.tobytes(), (name, comp, np.argwhere(pf.view(np.uint32) != stateless.view(np.uint32)).tolist()[:8])
            assert np.array_equal(pg, cases.group_sums(pf)) and np.array_equal(pg, eng.collapsed_loglik(0, comp))
            sums.append(pg)
        sums = np.concatenate(sums)
        assert np.array_equal(eng.collapsed_loglik_all(0), sums)
        per_group, per_object = eng.collapsed_and_source_prior(0)
        assert np.array_equal(per_group, sums) and np.array_equal(per_object, eng.source_prior(0))


@pytest.mark.parametrize("kind", ["moderate", "extreme"])
def test_a_step_at_the_ranges_concentrations_equals_the_stateless_call_on_its_counts(kind):
    s = cases.step_state(kind)
    with Engine(s.features, s.n_groups, n_slots=4) as eng:
        for comp in range(2):
            eng.set_concentration(comp, s.conc[comp])
        for slot in (0, 2):
            eng.load_state(slot, s.groups, s.weights, source=s.source)
            for comp in range(2):
                eng.update_probs(slot, comp)
            eng.mixture_loglik(slot)
        batch, _mix, _chg = eng.step_batch([0, 2], [1, 3], None, None, np.array([0, 2, 4], dtype=np.int32), np.tile(s.changed, 2),
                                           np.concatenate([s.rows, s.rows]))
        glh, _mix, changed = eng.step(0, 1, changed_objects=s.changed, source_rows=s.rows)
        assert changed[0] and changed[-1]                                    # out of the first cluster, into the confounder's group
        assert np.array_equal(batch[0], glh) and np.array_equal(batch[1], glh)             # k_step_core_batch: the same body
        for comp, (lo, hi) in enumerate(((0, s.n_groups[0]), (s.n_groups[0], s.n_groups[0] + 1))):
            counts = eng.get_counts(1, comp)
            assert not np.array_equal(counts, eng.get_counts(0, comp))
            pf, want = eng.dirichlet_logpdf(counts, s.conc[comp], per_group=True)
            assert np.array_equal(glh[lo:hi], want), (kind, comp)
            assert np.array_equal(eng.collapsed_loglik(1, comp), want)
            r = cases.assert_meets(cases.exact(counts, s.conc[comp]), pf, (kind, comp, "step"))
            print(cases.line(f"step {kind} component {comp}", r))
