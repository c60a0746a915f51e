"""Loader of tests/golden/wgibbs.npz (written by tests/golden/make_golden_wgibbs.py): the reference's recorded proposals of
GibbsSampleWeights._propose, per case a dict of the case's constants and a list of proposals with the packed arrays
unpacked -- shared by the CPU and the GPU tests of the Gibbs weights step."""
from pathlib import Path

import numpy as np

from tests import _wgibbs_oracle as worc

GOLDEN = Path(__file__).resolve().parent / "golden" / "wgibbs.npz"
CASES = ("cfg1", "south_america", "south_america_mc3", "south_america_symdir", "south_america_jeffreys", "south_america_bbs",
         "headline")
PER_PROPOSAL = ("w", "has_components", "src", "i12", "a2", "u", "beta_ab", "counts", "w_new", "log_lh_old", "log_lh_new",
                "log_prior_old", "log_prior_new", "log_q", "log_q_back", "p_accept", "accept", "w_out", "version")


def load(tag):
    with np.load(GOLDEN) as z:
        assert tuple(z["cases"]) == CASES
        n, f, c = (int(v) for v in z[f"{tag}/shape"])
        if f"{tag}/workload" in z.files:
            from sbayes_amd.synthetic import make_workload
            na = np.asarray(make_workload(str(z[f"{tag}/workload"])).na_values, dtype=bool)
        else:
            na = np.unpackbits(z[f"{tag}/na"])[:n * f].reshape(n, f).astype(bool)
        case = dict(tag=tag, shape=(n, f, c), na=na, prior_temperature=float(z[f"{tag}/prior_temperature"]),
                    prior_type=str(z[f"{tag}/prior_type"]), alpha=z[f"{tag}/alpha"],
                    concentration_array=z[f"{tag}/concentration_array"], proposals=[])
        stacked = {key: z[f"{tag}/{key}"] for key in PER_PROPOSAL}
    for k in range(stacked["w"].shape[0]):
        p = {key: stacked[key][k] for key in PER_PROPOSAL}
        p["has_components"] = np.unpackbits(p["has_components"])[:n * c].reshape(n, c).astype(bool)
        p["i1"], p["i2"] = (int(v) for v in p["i12"])
        p["src"] = p["src"].astype(np.int16)
        p["patterns"], p["pid"] = np.unique(p["has_components"], axis=0, return_inverse=True)
        p["pid"] = np.asarray(p["pid"]).reshape(-1)
        case["proposals"].append(p)
    return case


def source_array(src, n_components):
    """bool [N, F, C]: the one-hot source the engine takes, from the component index per observation (-1: none)."""
    return np.asarray(src)[..., None] == np.arange(n_components)


def oracle_step(case, p):
    """tests/_wgibbs_oracle.step on a recorded proposal: (weights_out, accept, terms, w_new)."""
    return worc.step(p["w"], p["patterns"], p["pid"], p["src"], case["na"], p["i1"], p["i2"], p["a2"], p["u"], case["alpha"],
                     p["beta_ab"], case["prior_temperature"])
