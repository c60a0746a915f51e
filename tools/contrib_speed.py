"""Speed of sbayes_amd.contribution at the two shapes of tools/ppc_speed.py (1000 objects x 200 features x 10 states, K = 5
clusters and one confounder of 10 groups; the south_america shape, 100 x 36 x 5, K = 3, two confounders of 1 and 6 groups),
T = 1000 samples each; prints one JSON line and writes it to --out.

Device: 2 warm-up and 5 timed repeats of evaluate() on all samples: the kernels' time by HIP events (preparation, validation,
cells and sums, summed over the library calls the block was split into) and the wall time of the synchronous call, smallest and
median, with the number of library calls; the upload (set_data) once.  Next to them, in the same session, the posterior
predictive check's check() at the same shape (sbayes_amd.ppc, without replicates): the yardstick for an equal tile plan.  And the
NumPy oracle (tests/_contrib_oracle.py) over --host-samples samples on the same host, with its seconds per sample and scaled to
T, and whether the device's sums of those samples lie in the band.
    python tools/contrib_speed.py [--samples 1000] [--out profiles/contrib/contrib_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import contribution, ppc             # noqa: E402
from tests import _contrib_oracle as orc             # noqa: E402
from tests import _predict_oracle as predict_orc     # noqa: E402

SHAPES = {"headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10]),
          "south_america": dict(N=100, F=36, S=5, C=3, K=3, group_counts=[1, 6])}
WARMUP, REPEATS = 2, 5
SEED = 2201


def timed(h, run, case, calls):
    walls, kernels = [], []
    for i in range(WARMUP + REPEATS):
        h.reset()
        t0 = time.perf_counter()
        run(case["clusters"], case["weights"], case["tables"])
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(h.kernel_ms)
    return {"kernel_ms": round(min(kernels), 4), "kernel_ms_median": round(float(np.median(kernels)), 4), "call_ms": round(min(walls), 4),
            "call_ms_median": round(float(np.median(walls)), 4), "library_calls": calls, "warmup": WARMUP, "repeats": REPEATS}


def worst_ratio(res, want, th):
    """The device's sums of the first th samples against the oracle's, in units of the band (+inf entries left out)."""
    worst = 0.0
    for got, ref, (terms, mag) in zip((res.affinity[:th], res.gain_feature[:th]), (want["affinity"], want["gain_feature"]), orc.terms_and_magnitudes(want)):
        finite = np.isfinite(ref)
        band = orc.band(terms, mag)
        ok = finite & (band > 0)
        worst = max(worst, float((np.abs(got - ref)[ok] / band[ok]).max()) if ok.any() else 0.0)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "contrib" / "contrib_speed.json")
    a = ap.parse_args()
    out = {"tool": "contrib_speed", "samples": a.samples, "runs": []}
    h, hp = contribution.ContributionHandle(0), ppc.PpcHandle(0)
    for name, shape in SHAPES.items():
        case = predict_orc.random_case(1, T=a.samples, out_share=0.2, na_share=0.05, **shape)
        t0 = time.perf_counter()
        h.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        run = {"shape": name, **{k: v for k, v in shape.items() if k != "group_counts"}, "R": shape["K"] + sum(shape["group_counts"]),
               "upload_ms": round((time.perf_counter() - t0) * 1e3, 3), "samples_per_library_call": h.max_samples()}
        run["evaluate"] = timed(h, h.evaluate, case, -(-a.samples // h.max_samples()))
        res = h.result()
        run["n_samples"], run["n_skipped"], run["rank"] = res.n_samples, res.n_skipped, res.rank()
        hp.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        run["ppc_check"] = timed(hp, lambda cl, w, tb: hp.check(cl, w, tb, seed=SEED), case, -(-a.samples // hp.max_samples()))
        th = min(a.host_samples, a.samples)
        part = {k: (v[:th] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}
        t0 = time.perf_counter()
        want = orc.evaluate(**part)
        seconds = time.perf_counter() - t0
        run["host"] = {"oracle_samples": th, "oracle_s_per_sample": round(seconds / th, 6), "oracle_s_scaled_to_samples": round(seconds / th * a.samples, 3),
                       "worst_band_ratio": worst_ratio(res, want, th)}
        out["runs"].append(run)
    h.close()
    hp.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
