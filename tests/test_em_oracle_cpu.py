"""The fp64 restatement of the EM initializer (tests/_em_oracle.py) against the reference's own generate_clusters_em,
recorded under fixed seeds in tests/golden/em_init.npz (tests/golden/make_golden_em.py).

Tolerance (from the arithmetic, not from the fixtures).  The reference runs each step in float32 (float64 with the
cost-based geo prior); _em_oracle.z_relative_bound gives, per step i, the relative error r_i of one such step's z from
its exact value: the logit error d_i = (F + 2) u (1 + max|ll|) / T_i (+ 2 (N + 2) u max|geo|), scaled by the softmax
into exp(2 d_i) - 1, plus (G + 3) u for the float32 softmax itself (u = 2^-24).  Every snapshot must be within 2 r_i
relative (one step's worth of error carried in from the steps before; a larger deviation would mean the EM map
amplifies float32 noise), with an absolute floor of the smallest normal float32 where the reference's z is float32.

Near-tie rule.  The final clusters must be equal except for objects whose decision margin (_em_oracle.decision_margin:
the relative gap to the nearest non-exact tie in discretize_fuzzy_cluster_2) is at most 2 r / (1 - r) with r = 2 r_49.
Objects below that bound per fixture (printed by test_near_tie_counts): cfg1 0, south_america 1, headline 0,
south_america_geo 0."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _em_oracle as orc  # noqa: E402

GOLDEN = np.load(HERE / "golden" / "em_init.npz")
CASES = ["cfg1", "south_america", "headline", "south_america_geo"]
NEAR_TIES = {"cfg1": 0, "south_america": 1, "headline": 0, "south_america_geo": 0}
F32_TINY = float(np.finfo(np.float32).tiny)


def case(tag):
    g = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(tag + "/")}
    g["cost"] = g.get("cost")
    g["scale"] = float(g["scale"]) if "scale" in g else None
    return g


_RUNS = {}


def restated(tag):
    if tag not in _RUNS:
        g = case(tag)
        rec = {}
        zs = orc.em_steps(g["x"], g["applicable"], g["groups_available"], int(g["n_clusters"]), g["z0"].astype(np.float64),
                          orc.temperatures(50), g["cost"], g["scale"], record=rec)
        _RUNS[tag] = (g, zs, rec)
    return _RUNS[tag]


def step_bound(g, rec, i):
    n, f = g["x"].shape
    return 2 * orc.z_relative_bound(f, g["groups_available"].shape[0], rec["ll_max"][i], orc.temperatures(50)[i], n,
                                    rec["geo_max"][i] if g["cost"] is not None else 0.0)


def assert_z_close(got, want, rel, floor, what):
    err = np.abs(got - want)
    bad = err > rel * np.abs(want) + floor
    assert not bad.any(), (f"{what}: {int(bad.sum())} entries beyond {rel:.3g} relative; worst "
                           f"{float((err / np.maximum(np.abs(want), floor)).max()):.3g}")


@pytest.mark.parametrize("tag", CASES)
def test_z_at_every_snapshot_within_float32_noise(tag):
    g, zs, rec = restated(tag)
    floor = F32_TINY if g["z"].dtype == np.float32 else 0.0
    assert g["z"].dtype == (np.float64 if g["cost"] is not None else np.float32)
    for j, step in enumerate(g["z_steps"]):
        assert_z_close(g["z"][j].astype(np.float64), zs[step], step_bound(g, rec, step), floor, f"{tag} step {step}")


@pytest.mark.parametrize("tag", CASES)
def test_final_clusters_equal_up_to_near_ties(tag):
    g, zs, rec = restated(tag)
    k, m, t = int(g["n_clusters"]), int(g["min_size"]), int(g["total_size"])
    z = zs[-1].astype(g["z"].dtype)
    got = orc.discretize(z, k, m, t)
    r = step_bound(g, rec, 49)
    near = orc.decision_margin(z, k, m, t) <= 2 * r / (1 - r)
    differ = (got != g["clusters"]).any(axis=0)
    assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)
    assert int(near.sum()) == NEAR_TIES[tag]


def test_discretize_restates_the_reference_on_its_own_z():
    """The restated discretization on the reference's own last z gives the reference's clusters."""
    for tag in CASES:
        g = case(tag)
        assert np.array_equal(orc.discretize(g["z"][-1], int(g["n_clusters"]), int(g["min_size"]), int(g["total_size"])),
                              g["clusters"]), tag


def test_fixture_is_small_and_complete():
    assert (HERE / "golden" / "em_init.npz").stat().st_size < 512 << 10
    for tag in CASES:
        g = case(tag)
        assert list(g["z_steps"]) == list(range(0, 50, 5)) + [49]
        assert g["z0"].dtype == np.float32 and g["z0"].shape == g["groups_available"].shape
        assert np.allclose(g["z0"].sum(axis=0), 1, atol=1e-6)
    assert case("headline")["groups_available"].shape == (6, 1000)


def test_bound_is_tight_enough_to_see_a_wrong_step():
    """The tolerance is not loose: dropping the NA column's log sum p (using log p of state 0 instead) breaks it."""
    g, zs, rec = restated("south_america")
    x = g["x"].copy()
    s = g["applicable"].shape[1]
    assert (x == s).any()
    x[x == s] = 0
    wrong = orc.em_steps(x, g["applicable"], g["groups_available"], int(g["n_clusters"]), g["z0"].astype(np.float64),
                         orc.temperatures(50))
    with pytest.raises(AssertionError):
        assert_z_close(g["z"][-1].astype(np.float64), wrong[49], step_bound(g, rec, 49), F32_TINY, "wrong NA column")
