"""The range cases of the normalised weights, the source prior and source_lh_by_feature (tests/_srcprior_range_cases.py) under the
NumPy oracle and mpmath alone: that each case reaches what it is there for -- 0, denormals and small normals at every place of
the row and every C from 1 to 8, every pattern the engine holds with the last pattern id among them, rows at C = 8 whose
chained float32 sum is not NumPy's, NaN and inf under a cleared and a set bit, masked sums of 0, the shape edges of the four
kernels, objects all NA / of one observation / with a 0xFF source / with sources of weight 0, 1, denormal and NaN, a grid of
normalised weights in every binade from 2^-149 to 1 -- and that the oracle itself lies inside the bands the device is held to
(tests/test_gpu_srcprior_range.py runs the cases on the device).  It measures L_ref, the worst error of NumPy's float32 log over
the grid in float32 ulps of the exact value, from which the oracle's own allowance ceil(max(1, L_ref)) and the device's, L_max =
min(that, 2), follow.

The oracle against the bands of the two sums: its float32 logs, summed EXACTLY and rounded once, lie inside the band taken with
the oracle's own allowance per log.  The oracle's own results do not all: it adds the logs in float32 -- np.sum over the
features pairwise, over the objects as a serial chain (oracle.source_lh_by_feature: up to N / 2 ulp) -- which the device does not
(float64 adds, one rounding).  They are held to the band plus that accumulation, (n - 1) u sum |log w|, and how far they leave
the device's band is printed: 3.3 to 13.7 bands at N >= 511 (F >= 15, C > 1).  That is a SERIAL float32 chain; the kernels' own lane
chain and tree with a float32 accumulator would stay inside the bands, and is seen by the E cases instead (last test)."""
import math
import re
from pathlib import Path

import mpmath
import numpy as np
import pytest

from tests import _srcprior_range_cases as sc
from tests._srcprior_range_cases import F32, FINITE, MIN_NORMAL, NAN, NINF, TINY, U

CSRC = Path(__file__).resolve().parent.parent / "sbayes_amd" / "csrc"


def _denormal(x):
    return (x > 0) & (x < F32(MIN_NORMAL))


# ---- W ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.group("W"))
def test_w_the_oracle_lies_inside_the_band_and_nothing_finite_is_left_out(name):
    c = sc.case(name)
    value, _band = sc.mp_normalized(c)
    d = sc.w_distance(c, c["wpat"])
    has = value != None                                                       # noqa: E711
    print(f"[srcprior-range] {name}: F x C {c['w'].shape}, {len(c['patterns'])} patterns, {c['hc'].shape[0]} rows, worst |oracle - mp| / band "
          f"{np.max(d[has], initial=0.0):.3g}, {int((~has).sum())} NaN entries")
    assert np.array_equal(has, np.isfinite(c["wpat"]))                        # every finite output has its 50-digit value
    assert np.isnan(c["wpat"][~has]).all()                                    # (no quotient is infinite: inf / inf is NaN)
    assert (d[has] <= 1.0).all()
    assert sc.bits_equal(c["want"], c["wpat"][c["pid"]])                      # the two forms of the oracle


def test_w_small_values_patterns_and_denormal_quotients():
    assert sc.SMALL == (0.0, 2.0 ** -149, 2.0 ** -126, 1e-30, 1e-20, 1e-10, 2.0 ** -24)
    for cc in range(1, 9):
        c = sc.case(f"W_small_c{cc}")
        w, pats, wpat = c["w"], c["patterns"], c["wpat"]
        assert set(c["rows"]) == {(v, k) for v in sc.SMALL for k in range(cc)}
        for r, (v, k) in enumerate(c["rows"]):
            assert w[r, k] == F32(v) and (np.delete(w[r], k) > 1e-3).all()    # ... beside ordinary weights
        assert len(pats) == sc.capacity(cc) == min(2 ** cc, 64)
        assert np.array_equal(np.unique(c["pid"]), np.arange(len(pats)))     # every pattern has a row: the last pattern id too
        if cc <= 4:
            assert len(pats) == 2 ** cc
        full, empty = int(np.flatnonzero(pats.all(axis=1))[0]), int(np.flatnonzero(~pats.any(axis=1))[0])
        assert np.isnan(wpat[empty]).all()                                    # a masked sum of 0: 0 / 0 everywhere
        for k in range(cc):                                                   # one present component: ordinary, denormal and 0
            p = int(np.flatnonzero((pats == (np.arange(cc) == k)).all(axis=1))[0])
            one = wpat[p, :, k]
            assert ((one == 1) | np.isnan(one)).all() and (np.delete(wpat[p], k, axis=1)[~np.isnan(one)] == 0).all()
            assert np.array_equal(np.isnan(one), w[:, k] == 0) and (one[_denormal(w[:, k])] == 1).all() and _denormal(w[:, k]).sum() >= 2
        # a flushed denormal -- an input, a sum or a quotient -- changes a compared entry
        assert _denormal(wpat).sum() >= cc or cc == 1                        # (at least 2^-149 at each place beside an ordinary weight)
        lo, hi = c["all_denormal"]
        assert _denormal(w[[lo, hi]]).all() and np.isfinite(wpat[full][[lo, hi]]).all() and (wpat[full][[lo, hi]] > 1e-4).all()
        if cc == 3:
            assert (wpat[full, lo] == F32(0.33333334)).all()                  # 2^-149 / (3 * 2^-149)
        if cc == 1:
            assert w[1, 0] == F32(TINY) and wpat[full, 1, 0] == 1             # 2^-149 / 2^-149


def test_w_the_sum_order_matters_at_eight_components():
    """On >= 64 rows of the wide case the quotients of a chained float32 sum are not the oracle's: a kernel that chains at C = 8 is seen."""
    c = sc.case("W_wide_c8")
    full = int(np.flatnonzero(c["patterns"].all(axis=1))[0])
    chained = sc.chained_normalize(c["w"], c["patterns"])
    differ = (chained[full] != c["wpat"][full]).any(axis=1)
    tree = lambda r: ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))     # noqa: E731
    for row in c["w"]:
        assert np.sum(row) == tree(row)                                       # NumPy's order at eight terms
    print(f"[srcprior-range] W_wide_c8: {int(differ.sum())} of {len(differ)} rows differ between the chain and NumPy's tree")
    assert differ.sum() >= 64 and c["n_differ"] >= 64 and (~differ).sum() >= 8
    assert c["w"].max() / c["w"].min() > 1e12
    for p in range(len(c["patterns"])):                                       # (fewer than eight terms under a set bit: 0 * w still counts)
        assert (chained[p] != c["wpat"][p]).any()


@pytest.mark.parametrize("cc", [4, 8])
def test_w_non_finite_weights_under_a_cleared_and_a_set_bit(cc):
    c = sc.case(f"W_nonfinite_c{cc}")
    pats, wpat, w = c["patterns"], c["wpat"], c["w"]
    zeroed = np.where(pats[:, None, :], w[None], F32(0))                      # what `0.0f` in place of `0.0f * w` would sum
    with np.errstate(invalid="ignore"):
        wrong = zeroed / zeroed.sum(axis=-1, keepdims=True)
    seen = {(kind, bit): 0 for kind in ("inf", "nan") for bit in (False, True)}
    for r, (v, k) in enumerate(c["rows"]):
        for p in range(len(pats)):
            seen[("nan" if math.isnan(v) else "inf", bool(pats[p, k]))] += 1
            if not pats[p, k] or math.isnan(v):                               # 0 * inf = NaN, or NaN itself, in the sum: the row is NaN
                assert np.isnan(wpat[p, r]).all()
                if not pats[p, k] and pats[p].any():
                    assert np.isfinite(wrong[p, r]).all()                     # ... which the zeroed form would not show
            else:                                                             # inf under a set bit: inf / inf and finite / inf
                assert np.isnan(wpat[p, r, k]) and (np.delete(wpat[p, r], k) == 0).all()
    assert all(n >= cc for n in seen.values()), seen
    assert np.isfinite(wpat[pats.any(axis=1), len(c["rows"])]).all()          # the plain row


def test_w_shapes_rows_and_the_row_form_limits():
    fc = [sc.case(f"W_f{f}_c{cc}")["w"].shape for f, cc in sc.W_SHAPES]
    assert {f for f, _ in fc} == {1, 15, 16, 17, 33} and {f * cc % 4 for f, cc in fc} == {0, 1, 2, 3} and min(f * cc for f, cc in fc) < 4
    assert {f * cc % 4 for f, cc in fc if f * cc > 4} == {0, 1, 2, 3}
    pf = {len(sc.case(n)["patterns"]) * sc.case(n)["w"].shape[0] for n in sc.group("W")}
    assert {255, 256, 257} <= pf and max(pf) > 2 * 256                        # P * F around the 256-thread block, and several blocks
    assert [sc.case(f"W_rows{n}")["hc"].shape[0] for n in sc.W_ROW_COUNTS] == [1, 7, 8, 9, 17, 300]
    assert sc.case("W_rows9")["w"].size % 4 == 3 and not sc.case("W_rows9")["slot_form"]
    # the limits as the launch code has them (sbe_normalize_weights): the constants alone, whatever stands around them
    launch = (CSRC / "sbe_engine_stateless.hip").read_text()
    body = launch[launch.index("int sbe_normalize_weights("):launch.index("int sbe_cluster_marginals(")]
    assert re.search(r"in_lds\s*=\s*w_lds\s*\+\s*kNwStaticLds\s*<=[^;]*\b64\s*<<\s*10", body) and re.search(r"\bN\s*<=\s*256\b", body)
    kernels = (CSRC / "sbe_kernels.hip.h").read_text()
    assert re.search(r"\bkNwRows\s*=\s*8\s*;", kernels) and re.search(r"\bkNwStaticLds\s*=\s*kNwRows\s*\*\s*sizeof\(uint32_t\)", kernels)
    assert sc.ROW_LDS_BUDGET == (64 << 10) - 8 * 4 and sc.ROW_MAPPED_LIMIT == 256 and 300 > sc.ROW_MAPPED_LIMIT
    big, full = sc.case("W_big_table"), sc.case("W_full_lds")
    f, cc = big["w"].shape
    assert cc == 8 and f * cc * 4 > sc.ROW_LDS_BUDGET >= (f - 1) * cc * 4     # the smallest F beyond the budget at C = 8
    assert full["w"].shape == (f - 1, cc) and full["w"].size * 4 + sc.ROW_STATIC_LDS == 64 << 10   # ... and the largest staged: 64 KB in all
    for c in (big, full):
        assert c["hc"].shape[0] == 9 and not c["slot_form"] and _denormal(c["w"][-8:]).any() and (c["w"][-8:] == 0).any()
    assert re.search(r"Pmax\s*=\s*std::min\(\s*1\s*<<\s*n_components\s*,\s*64\s*\)", (CSRC / "sbe_mixture_plan.h").read_text())
    s = sc.case("W_slot2_of_3")
    assert (s["n_slots"], s["slot"]) == (3, 2)


# ---- L_ref -------------------------------------------------------------------------------------------------------------------------
def test_the_grid_covers_every_binade_and_l_ref_is_measured():
    c = sc.case("P_grid")
    v = sc.grid_values(c)
    assert ((~c["na"]).sum(axis=1) == 1).all() and ((~c["na"]).sum(axis=0) == 1).all() and (v > 0).all() and (v <= 1).all()
    binade = np.floor(np.log2(v.astype(np.float64))).astype(int)
    for e in range(-149, 0):
        assert len(np.unique(v[binade == e])) >= (1 if e == -149 else 2 if e == -148 else 3), e
    for x in (F32(MIN_NORMAL), np.nextafter(F32(MIN_NORMAL), F32(0)), F32(TINY), F32(1), F32(1 - U)):
        assert (v == x).any(), x
    # ... and the log's own binades next to 0: -log w from 2^-24 up to 103
    with np.errstate(divide="ignore"):
        lb = np.floor(np.log2(-np.log(v[v < 1].astype(np.float64)))).astype(int)
    assert set(range(-24, 7)) <= set(lb.tolist())
    sums = sc.mp_sums(c, 1)
    assert all(s["cls"] == FINITE and s["n"] == 1 for s in sums)
    l_ref, at = sc.l_ref()
    print(f"[srcprior-range] L_ref = {l_ref:.3f} float32 ulp of the exact log (NumPy float32 log over {len(v)} weights, worst at w = {at!r} = "
          f"{float(at).hex()}); the oracle's allowance ceil(max(1, L_ref)) = {sc.l_oracle()}, the device's L_max = {sc.l_max()}")
    assert math.isfinite(l_ref) and sc.l_oracle() == math.ceil(max(1.0, l_ref)) and 1 <= sc.l_max() == min(sc.l_oracle(), 2)
    assert c["prior"][v == 1] == 0 and not np.signbit(c["prior"][v == 1]).any()


# ---- P and L ---------------------------------------------------------------------------------------------------------------------
def _oracle_sums(c, axis, label):
    """Classes equal the 50-digit ones; the oracle's float32 logs summed exactly and rounded once lie inside the band; the
    oracle's own float32 accumulation inside the band plus (n - 1) u sum |log w|."""
    got = c["prior"] if axis == 1 else c["by_feature"].astype(np.float64)
    cls = sc.sum_classes(c, axis)
    assert np.array_equal(sc.classes(got), cls), label
    picked, seen = (c["picked"], ~c["na"]) if axis == 1 else (c["picked"].T, ~c["na"].T)
    with np.errstate(divide="ignore", invalid="ignore"):
        logs = np.log(picked)
    assert logs.dtype == F32
    once = np.full(len(got), np.nan)
    accum = np.zeros(len(got))
    sums = sc.mp_sums(c, axis)
    for i in np.flatnonzero(cls == FINITE):
        once[i] = F32(math.fsum(logs[i][seen[i]].astype(np.float64).tolist()))
        accum[i] = max(sums[i]["n"] - 1, 0) * U * sums[i]["sum_abs"]
    fin = cls == FINITE
    lm = sc.l_oracle()                                                        # the oracle's own logs: its own allowance
    d_once, d_own = sc.s_distance(c, axis, once, lm), sc.s_distance(c, axis, got, lm, extra=accum)
    d_plain = sc.s_distance(c, axis, got, sc.l_max())                         # ... and against the band the device is held to
    print(f"[srcprior-range] {c['name']} {label}: classes finite/nan/+inf/-inf {'/'.join(map(str, sc.class_counts(cls)))}, worst / band: oracle's logs "
          f"summed exactly {np.max(d_once[fin], initial=0.0):.3g}, oracle {np.max(d_plain[fin], initial=0.0):.3g} (with its float32 accumulation "
          f"{np.max(d_own[fin], initial=0.0):.3g})")
    assert (d_once[fin] <= 1.0).all() and (d_own[fin] <= 1.0).all(), (c["name"], label)
    return d_plain


@pytest.mark.parametrize("name", sc.group("P"))
def test_p_the_oracle_lies_inside_the_band_and_the_kinds_are_what_they_claim(name):
    c = sc.case(name)
    _oracle_sums(c, 1, "prior")
    if "kinds" not in c:
        return
    prior, src, na, picked, fk = c["prior"], c["src"], c["na"], c["picked"], c["feature_kinds"]
    n, f = na.shape
    cc = c["w"].shape[1]
    for j, kind in enumerate(c["kinds"]):
        seen = ~na[j]
        if kind == "all_na":
            assert not seen.any() and prior[j] == 0 and not np.signbit(prior[j])
        elif kind == "single":
            assert seen.sum() <= 1
        elif kind == "no_source":
            assert (seen & (src[j] < 0)).sum() == 1 and prior[j] == -np.inf
        elif kind == "zero" and cc > 1 and f > 2:
            assert (picked[j][seen] == 0).any() and prior[j] == -np.inf
        elif kind == "denormal" and cc > 1 and f > 4:
            assert _denormal(picked[j][seen]).sum() == (fk == "denormal").sum() and math.isfinite(prior[j]) and prior[j] < -90
        elif kind == "nan" and f > 6:
            assert np.isnan(picked[j][seen]).any() and np.isnan(prior[j])
        elif kind == "one":
            assert c["hc"][j].sum() == 1 and (picked[j][seen] == 1).all() and prior[j] == 0 and not np.signbit(prior[j])
        elif kind == "last":
            assert (src[j][seen] == cc - 1).all() and (f < 15 or seen.sum() > f // 2)


def test_p_group_covers_the_shapes_the_kinds_and_the_value_classes():
    names = [n for n in sc.group("P") if n.startswith("P_f")]
    shapes = {(sc.case(n)["na"].shape[1], sc.case(n)["na"].shape[0]) for n in names}
    assert shapes == {(f, n) for f in (1, 63, 64, 65, 129) for n in (1, 15, 16, 17, 33)}
    assert {sc.case(n)["w"].shape[1] for n in names} == {1, 3, 8}
    for f in (1, 63, 64, 65, 129):                                            # every C at every F
        assert {sc.case(n)["w"].shape[1] for n in names if sc.case(n)["na"].shape[1] == f} == {1, 3, 8}
    counts = dict.fromkeys(sc.KINDS, 0)
    zero = one = den = nan = ff = 0
    for name in names:
        c = sc.case(name)
        seen = ~c["na"]
        for k in c["kinds"]:
            counts[k] += 1
        zero += int(((c["picked"] == 0) & seen & (c["src"] >= 0)).sum())
        ff += int((seen & (c["src"] < 0)).sum())
        one += int(((c["picked"] == 1) & seen).sum())
        den += int((_denormal(c["picked"]) & seen).sum())
        nan += int((np.isnan(c["picked"]) & seen).sum())
        if c["na"].shape[0] >= 15:
            assert set(sc.KINDS) <= set(c["kinds"].tolist())
    assert {str(sc.case(n)["kinds"][0]) for n in names if sc.case(n)["na"].shape[0] == 1} >= {"plain", "all_na", "zero"}
    assert min(counts.values()) >= 25 and min(zero, one, den, nan, ff) >= 25, (counts, zero, one, den, nan, ff)
    s = sc.case("P_slot2_of_3")
    assert (s["n_slots"], s["slot"]) == (3, 2) and s["na"].shape[1] % 64 != 0 and set(sc.sum_classes(s, 1).tolist()) == {FINITE, NAN, NINF}


@pytest.mark.parametrize("name", sc.L_CASES)
def test_l_the_oracle_lies_inside_the_band_and_the_features_are_what_they_claim(name):
    c = sc.case(name)
    d_plain = _oracle_sums(c, 0, "by feature")
    if "planned" not in c:
        return
    by, seen, picked = c["by_feature"], ~c["na"], c["picked"]
    n, f = c["na"].shape
    cc = c["w"].shape[1]
    if "all_na" in c["planned"]:
        j = c["planned"]["all_na"]
        assert not seen[:, j].any() and by[j] == 0 and not np.signbit(by[j])
    assert ("all_na" in c["planned"]) == (f > 1)
    if "single_ninf" in c["planned"]:
        j = c["planned"]["single_ninf"]
        assert ((picked[:, j] == 0) & seen[:, j]).sum() == 1 and by[j] == -np.inf and not np.isnan(picked[seen[:, j], j]).any()
    assert ("single_ninf" in c["planned"]) == (f > 2 and cc > 1 and n >= 15)
    cls = sc.sum_classes(c, 0)
    if f == 1:
        assert cls[0] == FINITE
    if f >= 15 and n >= 63:
        assert set(cls.tolist()) == {FINITE, NAN, NINF} and ((picked == 1) & seen).any()
        assert cc == 1 or (_denormal(picked) & seen).any()                    # (one component: a weight is 1, or NaN at 0 / 0)
        assert (seen & (c["src"] < 0)).any()                                  # a 0xFF source on an observed cell
    if n >= 511 and cc > 1 and f >= 15:
        # the oracle's serial float32 chain over the objects leaves the plain band: what a float32 accumulation in the kernel would show
        assert np.nanmax(d_plain) > 2.0, np.nanmax(d_plain)


def test_l_group_covers_the_shapes():
    shapes = [sc.case(n)["na"].shape for n in sc.group("L")]
    assert {n for n, _ in shapes} == {1, 63, 64, 65, 511, 512, 513, 1025} and {f for _, f in shapes} == {1, 15, 16, 17, 33}
    for n in (513, 1025):
        assert {f for m, f in shapes if m == n} == {1, 15, 16, 17, 33}
    assert sc.case("P_grid")["na"].shape[0] > 512                             # the grid state: two passes of 512 objects
    with mpmath.workdps(sc.MP_DIGITS):
        assert sc.mp_log(F32(1)) == 0 and abs(sc.mp_log(F32(0.5)) + mpmath.log(2)) < mpmath.mpf(10) ** -45


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def test_e_cases_give_the_logs_one_by_one_and_a_float32_accumulator_is_seen():
    """Every observation is the only one of its object (by feature) or of its feature (by object), everything is finite; the
    float64 sum of NumPy's float32 logs, rounded once, passes `exactly_rounded` for every sum, and the kernels' own lane chain
    and tree run with a float32 accumulator is rejected in 13 of the 27 sums by feature and 6 of the 36 by object."""
    rejected = {"feature": 0, "object": 0}
    total = dict(rejected)
    for name in sc.group("E"):
        c = sc.case(name)
        seen = ~c["na"]
        n, f = seen.shape
        assert (seen.sum(axis=1 if c["by"] == "feature" else 0) <= 1).all() and seen.sum(axis=0).all()
        assert (sc.sum_classes(c, 0) == FINITE).all() and (sc.sum_classes(c, 1) == FINITE).all()
        with np.errstate(divide="ignore"):
            logs = np.where(c["na"], F32(0), np.log(c["picked"]))
        for t in (logs.T if c["by"] == "feature" else logs):
            assert sc.exactly_rounded(F32(np.sum(t.astype(np.float64))), t)[0]
            rejected[c["by"]] += not sc.exactly_rounded(sc.float32_by_feature(t), t)[0]
            total[c["by"]] += 1
    print(f"[srcprior-range] E: a float32 lane chain and tree is rejected in {rejected} of {total} sums")
    assert rejected["feature"] >= 8 and rejected["object"] >= 4 and total == {"feature": 27, "object": 36}
    shapes = {(c["by"],) + c["na"].shape for c in map(sc.case, sc.group("E"))}
    assert ("feature", 1025, 1) in shapes and ("object", 1, 129) in shapes   # 1025 objects of one feature; 129 features of one object
