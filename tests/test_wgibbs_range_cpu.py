"""The range cases of the Gibbs weights step (tests/_wgibbs_range_cases.py) under tests/_wgibbs_oracle.py alone: that each case
reaches what it is there for -- zeros and float32 denormals at every place of the row and every C from 2 to 8, normalising
sums of 0, the ends of a2, alpha, A / B, T and u with coefficient 0 against an infinite log, the four classes of log_p with
their decisions, uniforms one float32 step from p, object counts around the sweep, 64 patterns over two feature tiles -- that
every finite feature decides more than twice the device band from its uniform (nothing is excluded on the device), and that
the oracle's log_p lies within a quarter of the band of a 50-digit evaluation of the contract.
tests/test_gpu_wgibbs_range.py runs the cases on the device."""
import numpy as np
import pytest

from tests import _wgibbs_oracle as worc
from tests import _wgibbs_range_cases as cases
from tests._wgibbs_range_cases import FINITE, NAN, NINF, PINF


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_finite_feature_decides_safely_and_the_oracle_agrees_with_50_digits(name):
    c = cases.case(name)
    fin = c["cls"] == FINITE
    dist = cases.distance_to_mp(c, c["terms"]["log_p"])
    least = np.min(c["margin"][fin] / np.maximum(c["band"][fin], 1e-300), initial=np.inf)
    print(f"[wgibbs-range] {name}: worst |oracle - mp| / band {np.max(dist[fin], initial=0.0):.3g}, least margin / band {least:.3g}, "
          f"classes finite/nan/+inf/-inf {'/'.join(map(str, cases.class_counts(c['cls'])))}")
    assert (c["margin"][fin] > 2 * c["band"][fin]).all()                      # nothing is excluded
    assert np.isfinite(c["band"][fin]).all() and np.isnan(dist[~fin]).all()
    assert (dist[fin] <= 0.25).all(), (name, np.flatnonzero(fin & ~(dist <= 0.25)).tolist())
    # the classes decide as the contract says, whatever u is
    assert not c["accept"][(c["cls"] == NAN) | (c["cls"] == NINF)].any() and c["accept"][c["cls"] == PINF].all()
    assert c["w_out"].tobytes() == np.where(c["accept"][:, None], c["w_new"], c["w"]).tobytes()
    if "built_for" in c:
        assert np.array_equal(c["cls"], c["built_for"]), np.flatnonzero(c["cls"] != c["built_for"]).tolist()
    else:
        assert fin.all()


def test_the_generator_refuses_a_uniform_within_twice_the_band():
    """float32(p) itself lies half a float32 step from p at the most: at N = 1541 that is inside twice the band for some feature."""
    c = cases.case("C_n1541_c4_below")
    log_p = c["terms"]["log_p"]
    p32 = np.exp(log_p).astype(np.float32)
    f = int(np.argmin(np.where(c["close"], worc.log_margin(p32, log_p) / c["band"], np.inf)))
    u = c["u"].copy()
    u[f] = p32[f]
    assert worc.log_margin(u, log_p)[f] <= 2 * c["band"][f]
    with pytest.raises(cases.Refused):
        cases.finish("refused", dict(cases.state_of(c), u=u))


# ---- A ------------------------------------------------------------------------------------------------------------------
def test_group_a_covers_every_c_pair_value_and_place():
    names = cases.group("A")
    assert len(names) == 2 + 6 + 12 + 4 * 3
    for cc in range(2, 9):
        pairs = {(c["i1"], c["i2"]) for c in map(cases.case, names) if c["w"].shape[1] == cc}
        if cc <= 4:
            assert pairs == {(a, b) for a in range(cc) for b in range(cc) if a != b}
        else:
            assert {(0, cc - 1), (cc - 1, 0)} < pairs and any(0 < a < cc - 1 and 0 < b < cc - 1 for a, b in pairs)
    assert cases.SMALL == (0.0, 2.0 ** -149, 2.0 ** -126, 1e-30, 1e-20, 1e-10, 2.0 ** -24)
    for name in names:
        c = cases.case(name)
        w, i1, i2, cc = c["w"], c["i1"], c["i2"], c["w"].shape[1]
        assert c["na"].shape[0] == cases.A_N and set(c["rows"]) == {(v, p) for v in cases.SMALL for p in cases.PLACES if p != "other" or cc > 2}
        for r, (v, place) in enumerate(c["rows"]):
            hit = w[r] == np.float32(v)
            want = {"i1": [i1], "i2": [i2], "both": [i1, i2]}.get(place)
            if want is None:
                assert hit.sum() == 1 and not hit[[i1, i2]].any()
            else:
                assert np.flatnonzero(hit).tolist() == sorted(want)
        assert (w[len(c["rows"]):] > 0.001).all()                             # the two plain rows


def test_group_a_zero_rows_reject_and_small_rows_show_their_proposal():
    for name in cases.group("A"):
        c = cases.case(name)
        for r, (v, place) in enumerate(c["rows"]):
            if (v, place) == (0.0, "both"):                                   # w02 = 0: a NaN a2_old, and at C = 2 a NaN row
                assert np.isnan(c["a2_old"][r]) and np.isnan(c["terms"]["log_p"][r])
                assert np.isnan(c["w_new"][r]).all() == (c["w"].shape[1] == 2)
                assert not c["accept"][r] and c["w_out"][r].tobytes() == c["w"][r].tobytes()
        # every other row has a finite log_p: at u = 0 it accepts whenever exp(log_p) > 0, and the device's w_new is compared
        with np.errstate(over="ignore"):
            shown = np.exp(c["terms"]["log_p"]) > 0
        assert shown.sum() >= 0.8 * len(shown), (name, int(shown.sum()))
        denormal = (c["w_new"] > 0) & (c["w_new"] < np.float32(2.0 ** -126))
        # a flushed float32 denormal changes a compared row (at C = 2 the row is the pair alone and normalises to normal numbers:
        # there the denormals are the products, their sum and the operands of the division)
        assert c["w"].shape[1] == 2 or denormal[shown].any(), name


def test_group_a_patterns_and_zero_normalising_sums():
    for name in cases.group("A"):
        c = cases.case(name)
        p, i1, i2 = c["patterns"], c["i1"], c["i2"]
        cc = p.shape[1]
        assert (~p[:, i1] & p[:, i2]).any() and (p[:, i1] & ~p[:, i2]).any() and p.all(axis=1).any()
        assert cc == 2 or (~p[:, i1] & ~p[:, i2]).any()
        assert np.array_equal(np.unique(c["pid"]), np.arange(len(p)))         # every pattern has objects
        with np.errstate(invalid="ignore", divide="ignore"):
            told = worc.normalized_weights(c["w"], p)
        zero_sum = np.isnan(told).all(axis=2)                                 # 0 / 0 on every component
        zero_sum[:, np.isnan(c["terms"]["log_p"])] = False
        assert zero_sum.any(), name                                           # ... in the table of a feature whose log_p is finite
        assert c["na"][zero_sum[c["pid"]]].all()                              # no observation reads such an entry


def test_the_row_sum_order_matters_at_eight_components():
    """The pairwise tree at C = 8 and the plain chain give different float32 sums on some proposed row of the C = 8 cases:
    a device that chains at eight is seen."""
    differ = 0
    for name in cases.group("A"):
        c = cases.case(name)
        if c["w"].shape[1] != 8:
            continue
        w02 = c["w"][:, c["i1"]] + c["w"][:, c["i2"]]
        t = c["w"].copy()
        t[:, c["i1"]] = (1 - c["a2"]) * w02
        t[:, c["i2"]] = c["a2"] * w02
        chain = np.zeros(len(t), dtype=np.float32)
        for k in range(8):
            chain = chain + t[:, k]
        with np.errstate(invalid="ignore"):
            differ += int(((t / chain[:, None]) != (t / np.sum(t, axis=-1, keepdims=True))).any(axis=1)[~np.isnan(chain)].sum())
    assert differ >= 8


# ---- B ------------------------------------------------------------------------------------------------------------------
def test_group_b_holds_every_class_and_every_value():
    names = cases.group("B")
    assert [cases.case(n)["t"] for n in names] == [1e-3, 1.0, 1.5, 1e3]
    for name in names:
        c = cases.case(name)
        cls, a2, u, ab, alpha = c["cls"], c["a2"], c["u"], c["beta_ab"], c["alpha"]
        assert all(k >= 8 for k in cases.class_counts(cls)), name
        fin = cls == FINITE
        assert set(cases.B_A2) <= set(a2[fin].tolist())                       # 0, 1 and the denormal among them
        assert set(np.float32(cases.B_U).tolist()) <= set(u[fin].tolist())
        assert set(cases.B_ALPHA) <= set(alpha[fin].ravel().tolist())
        assert (ab[fin] > 1e6 / c["t"]).any() and (ab[fin] == 1 + 0.5 / c["t"]).any()      # counts of 1e6 and of 0
        # coefficient 0 against an infinite log, in features whose log_p is finite
        with np.errstate(divide="ignore"):
            inf_a = np.isinf(np.log(a2)) | np.isinf(np.log(c["a2_old"].astype(np.float64)))
            inf_b = np.isinf(np.log1p(-a2)) | np.isinf(np.log1p(-c["a2_old"].astype(np.float64)))
            inf_w = np.isinf(np.log(c["w"])) | np.isinf(np.log(c["w_new"]))
        assert (fin & inf_a & (ab[:, 0] == 1)).sum() >= 2 and (fin & inf_b & (ab[:, 1] == 1)).sum() >= 2, name
        assert (fin & (a2 == 0) & (ab[:, 0] == 1)).any() and (fin & (a2 == 1) & (ab[:, 1] == 1)).any()
        assert (fin[:, None] & inf_w & (alpha == 1)).sum() >= 8, name
        assert (fin & (c["w"] == 0).any(axis=1)).any() and (fin & (c["w_new"] == 0).any(axis=1)).any()
        # the decisions of the classes at the uniforms that would show a wrong one
        assert (u[cls == NINF] == 0).all() and not c["accept"][cls == NINF].any()
        assert (u[cls == NAN] == 0).all() and not c["accept"][cls == NAN].any()
        assert (u[cls == PINF] == np.float32(1 - 2.0 ** -24)).all() and c["accept"][cls == PINF].all()
        for k in np.flatnonzero(cls == PINF):                                 # built as the contract's +inf
            seen = ~c["na"][:, k]
            assert seen.any() and (c["src"][seen, k] == c["i1"]).all() and a2[k] == 0
            assert alpha[k, c["i2"]] < 1 or ab[k, 0] > 1
        assert c["patterns"][:, c["i1"]].all()
        assert fin[c["accept"]].sum() >= 8 and (fin & ~c["accept"]).sum() >= 8


# ---- C ------------------------------------------------------------------------------------------------------------------
def test_group_c_uniforms_are_the_float32_neighbours_of_p():
    assert [s[1:] for s in cases.C_STATES] == [(37, 21, 3, None), (513, 17, 4, None), (1541, 50, 4, None), (1300, 33, 8, 40)]
    for name in cases.group("C"):
        c = cases.case(name)
        close, log_p, u = c["close"], c["terms"]["log_p"], c["u"]
        assert close.sum() >= 8, name
        p = np.exp(log_p)
        p32 = p.astype(np.float32)
        assert ((p32[close] > np.float32(2.0 ** -126)) & (p32[close] < 1)).all() and (u[~close] == 0.5).all()
        below, above = np.nextafter(p32, np.float32(-1)), np.nextafter(p32, np.float32(2))
        want = {"below": below, "above": above, "two_below": np.nextafter(below, np.float32(-1))}[c["side"]]
        assert np.array_equal(u[close], want[close])
        assert np.array_equal(c["accept"][close], np.full(close.sum(), c["side"] != "above"))
        assert (c["margin"][close] > 2 * c["band"][close]).all()
        # ... and no more than three float32 steps of p: an error of a few 1e-7 in log_p or in exp crosses it
        assert (c["margin"][close] < 3 * 2.0 ** -23).all()


# ---- D ------------------------------------------------------------------------------------------------------------------
def test_group_d_shapes_and_special_features():
    assert cases.D_N == (1, 511, 512, 513, 1023, 1025, 4099) and cases.D_F == (1, 15, 16, 17, 33)
    for n in cases.D_N:
        assert cases.case(f"D_n{n}")["na"].shape[0] == n
    assert cases.case("D_n4099")["w"].shape == (19, 2)
    for f in cases.D_F:
        assert cases.case(f"D_f{f}")["w"].shape[0] == f
    for cc in (7, 8):
        c = cases.case(f"D_p64_c{cc}")
        assert c["patterns"].shape == (64, cc) and c["w"].shape == (17, cc)  # 16 * 64 * 8 doubles: the LDS table at its limit
    c = cases.case("D_slot2_of_3")
    assert (c["n_slots"], c["slot"]) == (3, 2) and c["na"].shape[0] % 2 == 1
    for name in [f"D_n{n}" for n in cases.D_N] + ["D_p64_c7", "D_p64_c8", "D_slot2_of_3"]:
        c = cases.case(name)
        n = c["na"].shape[0]
        seen = ~c["na"]
        for j, kind in enumerate(c["special"]):
            if kind == "all_na":
                assert not seen[:, j].any() and c["terms"]["d_lh"][j] == 0 and c["terms"]["log_p"][j] != 0
            elif kind == "last_object_only":
                assert np.flatnonzero(seen[:, j]).tolist() == [n - 1]
            else:
                comp = c["i1"] if kind == "all_i1" else c["i2"]
                assert (c["src"][seen[:, j], j] == comp).all() and (n < 100 or seen[:, j].sum() > n // 4)


def test_a_permutation_of_the_features_permutes_the_oracle():
    c = cases.case(cases.PLACE_CASE)
    f = c["w"].shape[0]
    assert f > 16 + 5                                                         # two tiles; a rotation by 5 crosses their edge
    order = np.roll(np.arange(f), 5)
    r = cases.finish(c["name"], cases.replaced(c, order))
    assert r["w_out"].tobytes() == c["w_out"][order].tobytes() and np.array_equal(r["accept"], c["accept"][order])
    fin = r["cls"] == FINITE                                                  # (NumPy's own sum over the objects depends on the layout)
    assert np.array_equal(r["cls"], c["cls"][order]) and (np.abs(r["terms"]["log_p"] - c["terms"]["log_p"][order])[fin] <= r["band"][fin]).all()
