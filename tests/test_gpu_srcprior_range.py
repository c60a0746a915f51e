"""Device against oracle and against 50-digit values for the per-pattern normalised weights, the per-object source prior and
source_lh_by_feature, where the fixtures do not reach.  The cases are tests/_srcprior_range_cases.py; tests/test_srcprior_range_cpu.py
proves under the oracle and mpmath alone what each is there for and measures L_ref.  DESIGN.md section 4.3c.

    normalisation   k_weight_patterns / k_scatter_weight_patterns (one item function), k_expand_weights     set_weights after set_groups / set_groups
                                                                                                           after set_weights, weights_normalized(slot)
                    k_normalize_weight_rows, both stage_weights branches                                   Engine.normalize_weights
    source prior    k_source_prior, the object blocks of k_collapsed_source_prior                          source_prior(slot),
                                                                                                           collapsed_and_source_prior(slot)[1]
    by feature      k_source_lh_by_feature                                                                 source_lh_by_feature(slot)

Normalisation.  Both forms are the oracle's bit for bit (NaN where NaN) and each other's, and every finite entry is within the
band of the 50-digit quotient of the float32 weights as stored.  The band: m_c = w_c under a set bit, 0 * w_c under a cleared
one, all >= 0, S = sum m.  A float32 addition rounds once, relative u = 2^-24, and is exact where its result is denormal, so
whatever the order the computed sum is S (1 + d), |d| <= g = (C - 1) u / (1 - (C - 1) u): (C - 1) u relative to the sum of the
magnitudes, no absolute floor.  The division rounds once: u relative, or half a denormal step where the quotient is denormal.  So
    |out - m_c / S| <= (m_c / S) (g + u (1 + g)) + 2^-149.
A floor of 2^-149 on the sum as well would be wider for nothing (three weights of 2^-149 are held to 1/3 within 3 u here, and
would be within 1/3 of it there).  A row whose masked values hold an inf has S = inf: its finite quotients are exactly 0.

Source prior and source_lh_by_feature.  Classes (finite, NaN, +inf, -inf) equal the oracle's; an object that is NA throughout
gives +0.0 bit for bit; source_prior(slot) and collapsed_and_source_prior(slot)[1] are bit-equal.  A finite sum is held to
    |out - exact| <= sum L_max ulp32(|log w|) + 1/2 ulp32(|exact|) + n 2^-53 sum |log w|,      n = F (prior) or N (by feature),
`exact` the 50-digit sum of the logs of the float32 normalised weights as the oracle rounds them (the device's are the same
bits, asserted above): every float32 logf within L_max ulp of the exact log, at most n float64 additions on a term's way, one
rounding to float32.  L_max = min(ceil(max(1, L_ref)), 2), L_ref the worst error of NumPy's float32 log over the grid (measured by
the CPU test, never from the device): the device's logf may be as inexact as the reference's and no worse -- and no worse than the
2 ulp expected of a float32 log where the reference needs more (it needs 3 on this grid, which holds weights next to 1 beside
every binade from 2^-149 up; on the binades alone it needs 1).  L_max follows the host's NumPy: one with a more accurate float32
log tightens it.  On the grid every
object has one observation, so the output IS float(logf(w)): L_dev, the worst |out - log w| in float32 ulps of the exact log,
is printed and held to L_max.  The oracle's own sums are not the reference here: it adds float32 logs in float32.

Which test fails under which change of the kernels (reasoned from the code, not run):
    a chained sum at C = 8 (np_pairwise_sum)      test_normalisation[W_wide_c8]: 96 rows whose chained quotients differ (CPU-asserted); also
                                                  W_small_c8, W_f33_c8, W_big_table, bit for bit
    `0.0f` in place of `0.0f * w[c]`              test_normalisation[W_nonfinite_c4], [W_nonfinite_c8]: NaN / inf under a cleared bit, the
                                                  whole row NaN in the oracle, finite in the changed kernel
    a flushed denormal input, sum or quotient;    test_normalisation[W_small_c*] (2^-149 at every place, the all-denormal rows, 2^-149 /
    a division that is not correctly rounded      2^-149 = 1, 1/3), bit for bit
    a fast or flushing logf                       test_source_prior[P_grid] and test_source_lh_by_feature[P_grid]: L_dev; 88 weights of the
                                                  grid are denormal (a flushed one gives -inf against a finite class)
    float32 accumulation                          test_a_sum_is_the_float64_sum_of_the_device_logs_rounded_once: the E cases, where one kernel
                                                  returns the device's logs one by one and the other's sum must be their float64 sum rounded
                                                  once.  The kernels' own lane chain and tree with a `float` accumulator fail 13 of the 27 sums
                                                  of k_source_lh_by_feature and 6 of the 36 of k_source_prior (simulated by the CPU test).  The
                                                  BANDS do not catch it: such a chain and tree stays at 0.28 to 0.40 of the band at N = 1025 and
                                                  at F = 129 (a few roundings of half an ulp of the sum against the logs' L_max ulp each); only
                                                  a SERIAL float32 chain over the objects, the oracle's own sum, leaves them (3.3 to 13.7 bands
                                                  at N >= 511)
    a dropped `n < N` guard                       k_source_prior: an out-of-bounds write (N = 1, 15, 17, 33 are no multiple of the 16
                                                  objects of a block) -- not a test's business to provoke; k_source_lh_by_feature: the
                                                  clamped object N - 1 counted again, every finite band at N off 512; k_normalize_weight_rows:
                                                  rows 1, 7, 9, 17 (writes past the result)
    a dropped `f < F` guard                       k_source_lh_by_feature writes past `out` at F off 16; `f < F` in the lane loop of
                                                  source_prior_block: F = 1, 63, 65, 129 read the padding or the next row (NA bytes: skipped)
                                                  or the next feature's weights: bands and classes
    a dropped NA skip                             the all-NA objects (+0.0 asked, log of a weight read at source 0xFF -> -inf) and the
                                                  whole-NA feature
    a dropped `sc >= C` / `c < C` override        the 0xFF sources on observed cells: -inf asked; the clamped read gives the last
                                                  component's weight (k_source_lh_by_feature) or reads behind the row (k_source_prior)
    a block offset that ignores G                 test_source_prior[*_c3], [*_c8]: the fused launch's object block 0 at block index G = C
                                                  would be taken for block G: objects shifted by 16 G, the first 16 G never written
    the float4 staging tail dropped               test_normalisation at F * C mod 4 != 0, row form (W_rows*: F * C = 51)
    a slot offset dropped                         W_slot2_of_3, P_slot2_of_3 (slot 0 holds another state)

The stage_weights == 0 branch of k_normalize_weight_rows is taken when F * C * 4 + 32 > 64 KB (sbe_normalize_weights); nothing the engine
exposes says which branch ran, so W_big_table is sized from that constant less the kernel's 32 static bytes (F = 2048 at C = 8,
the smallest; the CPU test reads the constants in the source).  Nothing reads wpat_t, the float64 transposed copy of the normalised weights that the fused mixture
kernels consume, but those kernels: it is an exact widening written in the same lambda as wpat (weight_patterns_item) and is
covered only through its consumers' tests.  Likewise nothing says whether set_groups after set_weights wrote the normalised
weights in its own launch (k_scatter_weight_patterns: upload_segments takes it when the slot's staged arrays -- pattern ids, pattern
bits, tuple tables, one component's group ids -- are at most 8 and fit 64 KB of the mapped ring together) or fell back to
k_weight_patterns: by that condition the cases, of at most 104 objects, take the launch, but no test can tell.  W_full_lds
(F = 2047 at C = 8) is the largest table the row kernel stages: 65 504 bytes beside its 32 static ones, 64 KB in all."""
import numpy as np
import pytest

from tests import _srcprior_range_cases as sc
from tests._srcprior_range_cases import FINITE
from tests.test_gpu_wgibbs import bind, make_engine

pytestmark = pytest.mark.gpu


# ---- normalisation -----------------------------------------------------------------------------------------------------------------
def _engine_w(c, regroup=False):
    """An engine of the case's F and C; for the slot form its objects are the case's rows.  Another slot holds another state.
    `regroup`: the slot gets other groups first, then the weights, then the case's groups -- the normalised weights are then
    written by the set_groups launch (k_scatter_weight_patterns) instead of set_weights' (k_weight_patterns)."""
    f, cc = c["w"].shape
    n = c["hc"].shape[0] if c["slot_form"] else 1
    eng = make_engine(np.zeros((n, f), dtype=bool), cc, n_slots=c["n_slots"])
    if c["slot_form"]:
        other = [(0, ~c["hc"], c["w"][::-1])] if c["slot"] != 0 else []
        for slot, hc, w in other + [(c["slot"], ~c["hc"] if regroup else c["hc"], c["w"])]:
            for comp in range(cc):
                eng.set_groups(slot, comp, hc[:, comp][None, :])
            eng.set_weights(slot, w)
        if regroup:
            for comp in range(cc):
                eng.set_groups(c["slot"], comp, c["hc"][:, comp][None, :])
    return eng


def _normalise(c):
    """(row form, slot form or None) of one call each on a fresh engine, and of a second call on it."""
    with _engine_w(c) as eng:
        return [(eng.normalize_weights(c["w"], c["hc"]), eng.weights_normalized(c["slot"]) if c["slot_form"] else None) for _ in range(2)]


@pytest.mark.parametrize("name", sc.group("W"))
def test_normalisation(name):
    c = sc.case(name)
    (rows, slot), _ = _normalise(c)
    worst = sc.w_row_distance(c, rows)
    worst_slot = sc.w_row_distance(c, slot) if slot is not None else 0.0
    same = sc.bits_equal(rows, c["want"]), slot is None or sc.bits_equal(slot, c["want"])
    print(f"[srcprior-range] {name}: F x C {c['w'].shape}, {len(c['patterns'])} patterns, {c['hc'].shape[0]} rows, worst |dev - mp| / band: row form "
          f"{worst:.3g}, slot form {worst_slot:.3g}; bit-equal to the oracle: row form {same[0]}, slot form {same[1] if slot is not None else '-'}; "
          f"{int(np.isnan(c['want']).sum())} NaN entries")
    assert rows.dtype == np.float32 and rows.shape == c["want"].shape
    assert same[0], name                                                      # bit for bit, NaN where NaN
    assert worst <= 1.0
    if slot is not None:
        assert same[1] and sc.bits_equal(slot, rows) and worst_slot <= 1.0, name
        with _engine_w(c, regroup=True) as eng:                               # ... and written by the set_groups launch
            assert sc.bits_equal(eng.weights_normalized(c["slot"]), c["want"]), name


# ---- source prior and source_lh_by_feature ---------------------------------------------------------------------------------------
def _engine_s(c, collapsed=False):
    eng = make_engine(c["na"], c["w"].shape[1], n_slots=c["n_slots"])
    if c["slot"] != 0:                                                        # another state in slot 0
        bind(eng, 0, ~c["hc"], np.where(c["src"] > 0, 0, c["src"]), c["w"][::-1])
    bind(eng, c["slot"], c["hc"], c["src"], c["w"])
    if collapsed:                                                             # what the fused call's group blocks read
        f = c["na"].shape[1]
        for comp in range(c["w"].shape[1]):
            eng.set_concentration(comp, np.ones((f, 2)))
        eng.recount(c["slot"])
    return eng


def _check_sums(c, axis, got, label):
    want = c["prior"] if axis == 1 else c["by_feature"]
    cls = sc.sum_classes(c, axis)
    fin = cls == FINITE
    dist = sc.s_distance(c, axis, got, sc.l_max())
    print(f"[srcprior-range] {c['name']} {label}: N x F {c['na'].shape}, C {c['w'].shape[1]}, classes finite/nan/+inf/-inf "
          f"{'/'.join(map(str, sc.class_counts(sc.classes(got))))}, worst |dev - mp| / band {np.max(dist[fin], initial=0.0):.3g} (L_max {sc.l_max()}), "
          f"largest |dev - oracle| {np.max(np.abs(got[fin] - want[fin]), initial=0.0):.3g}")
    assert np.array_equal(sc.classes(got), sc.classes(want)) and np.array_equal(sc.classes(got), cls), label
    assert np.array_equal(got[fin].astype(np.float32).astype(got.dtype), got[fin])                 # float32 values
    assert (dist[fin] <= 1.0).all(), (label, np.flatnonzero(fin & ~(dist <= 1.0)).tolist())
    return dist


def _grid(c, got, label):
    l_dev, at = sc.log_ulps(sc.grid_values(c), got)
    l_ref, ref_at = sc.l_ref()
    print(f"[srcprior-range] {label}: L_dev = {l_dev:.3f} float32 ulp of the exact log over {len(got)} weights (worst at w = {float(at).hex()}); "
          f"L_ref = {l_ref:.3f} (w = {float(ref_at).hex()}), L_max = {sc.l_max()}")
    assert l_dev <= sc.l_max(), (l_dev, at)


@pytest.mark.parametrize("name", sc.group("P"))
def test_source_prior(name):
    c = sc.case(name)
    with _engine_s(c, collapsed=True) as eng:
        normalised = eng.weights_normalized(c["slot"])
        got = eng.source_prior(c["slot"])
        per_group, fused = eng.collapsed_and_source_prior(c["slot"])
        groups_alone = eng.collapsed_loglik_all(c["slot"])
    assert sc.bits_equal(normalised, c["wn"])                                 # the weights the sums are taken over: the oracle's bits
    _check_sums(c, 1, got, "source_prior")
    assert got.dtype == np.float64 and sc.bits_equal(got, fused)              # the object blocks behind the G group blocks
    assert sc.bits_equal(per_group, groups_alone)
    all_na = c["na"].all(axis=1)
    assert (got[all_na].view(np.uint64) == 0).all()                           # +0.0
    if name == "P_grid":
        _grid(c, got, "k_source_prior")


@pytest.mark.parametrize("name", sc.L_CASES)
def test_source_lh_by_feature(name):
    c = sc.case(name)
    with _engine_s(c) as eng:
        got = eng.source_lh_by_feature(c["slot"])
    assert got.dtype == np.float32
    _check_sums(c, 0, got, "source_lh_by_feature")
    all_na = c["na"].all(axis=0)
    assert (got[all_na].view(np.uint32) == 0).all()                           # +0.0
    if name == "P_grid":
        _grid(c, got, "k_source_lh_by_feature")


# ---- the accumulation, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.group("E"))
def test_a_sum_is_the_float64_sum_of_the_device_logs_rounded_once(name):
    """One kernel returns the device's float32 logs one by one (every object, or every feature, has one observation), the other
    adds them: its result is float32(math.fsum(those logs)) -- or the neighbour where the exact sum lies within the float64
    adds' own error of a rounding tie.  A float32 accumulator in the lane chain or the tree fails this in 13 of the 27 sums by
    feature and 6 of the 36 by object (tests/test_srcprior_range_cpu.py runs that simulation)."""
    c = sc.case(name)
    with _engine_s(c) as eng:
        prior, by = eng.source_prior(c["slot"]), eng.source_lh_by_feature(c["slot"])
    _check_sums(c, 1, prior, "source_prior")
    _check_sums(c, 0, by, "source_lh_by_feature")
    seen = ~c["na"]
    if c["by"] == "feature":
        sums, rows = by, [np.where(seen[:, f], prior, 0.0) for f in range(seen.shape[1])]
    else:
        sums, rows = prior, [np.where(seen[n], by.astype(np.float64), 0.0) for n in range(seen.shape[0])]
    results = [sc.exactly_rounded(got, terms) for got, terms in zip(sums, rows)]
    off = [abs(float(got) - exact) / float(sc.ulp32(exact)) for got, (_, exact) in zip(sums, results)]
    print(f"[srcprior-range] {name}: {len(results)} sums of up to {max(int((r != 0).sum()) for r in rows)} device logs, "
          f"{sum(ok for ok, _ in results)} exactly rounded, largest distance from the exact sum {max(off):.3f} ulp")
    assert all(ok for ok, _ in results), (name, [i for i, (ok, _) in enumerate(results) if not ok])


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W_small_c8", "W_big_table"])
def test_two_normalisations_of_the_same_state_return_the_same_bits(name):
    first, second = _normalise(sc.case(name))
    for a, b in zip(first, second):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["P_f129_n33_c8", "L_n1025_f33_c8"])
def test_two_calls_on_the_same_state_return_the_same_bits(name):
    c = sc.case(name)
    with _engine_s(c, collapsed=True) as eng:
        runs = [(eng.source_prior(c["slot"]), eng.collapsed_and_source_prior(c["slot"])[1], eng.source_lh_by_feature(c["slot"])) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
