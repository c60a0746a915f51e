"""The recorded cases of tests/golden/geo_prior.npz (tests/golden/make_golden_geo.py) and the comparisons both the CPU
test of the oracle and the GPU test of the device run against them, at the bounds tests/_geo_oracle.py derives."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from tests import _geo_oracle as orc

REPO = Path(__file__).resolve().parent.parent
CASES = ["south_america", "synthetic", "duplicates", "ties", "all_zero", "single", "pair", "whole"]
SKELETONS, AGGREGATIONS, PROBABILITY_FUNCTIONS = orc.SKELETONS, orc.AGGREGATIONS, orc.PROBABILITY_FUNCTIONS


def load():
    with np.load(REPO / "tests" / "golden" / "geo_prior.npz", allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    cases = {}
    for key, value in flat.items():
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = value
    for c in cases.values():
        if "cost" not in c:
            c["cost"] = orc.euclidean_cost(c["xy"])
    return cases


def oracle_skeletons(c):
    """{skeleton: dict of arrays [B]} of a case's masks."""
    out = {}
    for sk in SKELETONS:
        rows = [orc.skeleton(c["cost"], mk, sk) for mk in c["masks"]]
        out[sk] = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    return out


def check_skeleton_against_fixture(got, c, label):
    """got: {skeleton: object or dict with m, n_edges, sum, max}.  Integers and max equal what the reference's skeleton
    held; the sum within sum_bound of np.sum over it."""
    for s, sk in enumerate(SKELETONS):
        g = got[sk]
        get = (lambda k: np.asarray(g[k])) if isinstance(g, dict) else (lambda k: np.asarray(getattr(g, k)))
        assert np.array_equal(get("m"), c["masks"].sum(axis=1)), (label, sk)
        assert np.array_equal(np.maximum(get("n_edges"), 1), c["edges_size"][s]), (label, sk)
        assert np.array_equal(get("max"), c["edges_max"][s]), (label, sk)
        err = np.abs(get("sum") - c["edges_sum"][s])
        bound = orc.sum_bound(get("n_edges")) * c["edges_sum"][s]
        print(f"{label} {sk}: sum against the reference: largest error {float(err.max()):.3g} (bound there "
              f"{float(bound[np.argmax(err)]):.3g})")
        assert np.all(err <= bound), (label, sk, err, bound)


def check_prior(got, want, c, skeletons, libm, reference_form, label):
    """got, want: [2, 3, 2, B] log priors; skeletons: oracle_skeletons(c), whose aggregates and edge counts size the bound."""
    worst = 0.0
    for s, sk in enumerate(SKELETONS):
        for a, agg in enumerate(AGGREGATIONS):
            x = skeletons[sk][agg]
            rel = orc.aggregate_bound(agg, skeletons[sk]["n_edges"])
            for p, pf in enumerate(PROBABILITY_FUNCTIONS):
                bound = orc.probability_bound(x, rel, pf, c["scale"][a], c["x0"][a], libm=libm, reference_form=reference_form)
                err = np.abs(got[s, a, p] - want[s, a, p])
                assert np.all(np.isfinite(got[s, a, p])), (label, sk, agg, pf)
                if agg == "max" and pf == "exponential":
                    assert np.array_equal(got[s, a, p], want[s, a, p]), (label, sk)
                worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
                assert np.all(err <= bound), (label, sk, agg, pf, err, bound)
    print(f"{label}: log prior: largest error / bound {worst:.3g}")


def check_per_object(got, want, c, mst, libm, reference_form, label):
    """got, want: [3, 2, B, N]; mst: oracle_skeletons(c)["mst"]."""
    worst = 0.0
    for a, agg in enumerate(AGGREGATIONS):
        for p, pf in enumerate(PROBABILITY_FUNCTIONS):
            for i, mk in enumerate(c["masks"]):
                ctc = c["cost"][mk].min(axis=0)
                bound = orc.costs_per_object_bound(ctc, int(mst["m"][i]), mst[agg][i], mst["n_edges"][i], agg, pf, c["scale"][a],
                                                   c["x0"][a], libm=libm, reference_form=reference_form)
                err = np.abs(got[a, p, i] - want[a, p, i])
                worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(float).tiny))))
                assert np.all(err <= bound), (label, agg, pf, i, float(err.max()), float(bound[np.argmax(err)]))
    print(f"{label}: costs per object: largest error / bound {worst:.3g}")
