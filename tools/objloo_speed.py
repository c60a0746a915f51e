"""Speed of sbayes_amd.objloo at the south_america shape (100 objects x 36 features x 5 states, two confounders of 1 and 6 groups)
and at the headline shape (1000 x 200 x 10, one confounder of 10 groups), K = 5 clusters and T = 1000 samples each; prints one JSON
line and writes it to --out.

Per shape, in one process, 1 warm-up and 3 timed repeats of each, the variants of one repeat run one after the other (alternating):
  objloo        the three phases from an empty store: add, weights, accumulate, then the read: the kernels' time by HIP events,
                summed over the library calls a pass was split into, and the wall time of the synchronous calls;
  contribution  evaluate on the same inputs (affinity and gain): phase 1 forms the same K + 1 logs per cell, so it is reported
                against this;
  loopred       its three phases on the same inputs: the per-cell unit this one stands beside.
Smallest and median of the repeats.  Host: the NumPy checker (tests/_objloo_oracle.py) over the first --host-objects objects and
the first --host-samples samples, scaled to the N objects and T samples (its PSIS is per object and grows with T log T; the scaling is
linear, so the figure is a lower estimate).
    python tools/objloo_speed.py [--samples 1000] [--out profiles/objloo/objloo_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import contribution, loopred, objloo    # noqa: E402
from tests import _objloo_oracle as orc                 # noqa: E402
from tests import _predict_oracle as po                 # noqa: E402

SHAPES = {"south_america": dict(N=100, F=36, S=5, C=3, K=5, group_counts=[1, 6]),
          "headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10])}
WARMUP, REPEATS = 1, 3
SAMPLES = ("clusters", "weights", "tables")


def make_case(shape, T):
    """A seeded case whose observed cells have a confounder and a positive likelihood in every sample: every object is in a group
    of the first confounder (a fifth of them are in no cluster of a sample)."""
    case = po.random_case(1, T=T, out_share=0.2, na_share=0.05, **shape)
    first = case["groups"][0]
    first[first == po.NA] = 0
    return case


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(values):
    return {"min": round(min(values), 4), "median": round(float(np.median(values)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--host-objects", type=int, default=4)
    ap.add_argument("--host-samples", type=int, default=100)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "objloo" / "objloo_speed.json")
    a = ap.parse_args()
    T = a.samples
    out = {"tool": "objloo_speed", "samples": T, "warmup": WARMUP, "repeats": REPEATS, "runs": []}
    for name, shape in SHAPES.items():
        case = make_case(shape, T)
        samples = tuple(case[k] for k in SAMPLES)
        data = (case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        h, c, lp = objloo.ObjLooHandle(0), contribution.ContributionHandle(0), loopred.LooPredHandle(0)
        h.set_data(*data, capacity=T)
        c.set_data(*data)
        lp.set_data(*data, capacity=T)
        names = ("add", "weights", "accumulate")
        times = {k: [] for k in [f"{n}_{w}" for n in names for w in ("call", "kernel")] + ["read_call", "contrib_call", "contrib_kernel"] +
                 [f"loopred_{n}_{w}" for n in names for w in ("call", "kernel")]}
        for i in range(WARMUP + REPEATS):
            rec = {}
            h.reset()
            rec["add_call"], _ = wall(lambda: h.add(*samples))
            rec["add_kernel"] = h.kernel_ms["add"]
            rec["weights_call"], (pointwise, membership) = wall(h.weights)
            rec["weights_kernel"] = h.kernel_ms["weights"]
            rec["accumulate_call"], _ = wall(lambda: h.accumulate(*samples))
            rec["accumulate_kernel"] = h.kernel_ms["accumulate"]
            rec["read_call"], (p_loo, n_done) = wall(h.sums)
            c.reset()
            rec["contrib_call"], _ = wall(lambda: c.evaluate(*samples))
            rec["contrib_kernel"] = c.kernel_ms
            lp.reset()
            rec["loopred_add_call"], _ = wall(lambda: lp.add(*samples))
            rec["loopred_weights_call"], _ = wall(lp.weights)
            rec["loopred_accumulate_call"], _ = wall(lambda: lp.accumulate(*samples))
            for n in names:
                rec[f"loopred_{n}_kernel"] = lp.kernel_ms[n]
            if i >= WARMUP:
                for k, v in rec.items():
                    times[k].append(v)
        assert n_done == T and np.isfinite(p_loo).all() and np.isfinite(pointwise[0]).all() and np.allclose(membership.sum(axis=1), 1.0, atol=1e-9)
        run = {"shape": name, **{k: v for k, v in shape.items() if k != "group_counts"}, "R": shape["K"] + sum(shape["group_counts"]),
               "store_bytes": objloo.store_bytes(shape["N"], shape["K"], T), "library_calls_per_pass": -(-T // h.max_samples()),
               "contrib_library_calls": -(-T // c.max_samples()), "ms": {k: stats(v) for k, v in times.items()},
               "elpd": round(float(pointwise[0].sum()), 3), "elpd_cond": round(float(pointwise[4].sum()), 3),
               "n_bad_k": int((~(pointwise[1] <= 0.7)).sum()), "n_bad_k_cond": int((~(pointwise[5] <= 0.7)).sum())}
        ms = run["ms"]
        run["add_kernel_over_contrib_kernel"] = round(ms["add_kernel"]["min"] / ms["contrib_kernel"]["min"], 3)
        h.close()
        c.close()
        lp.close()
        n_host, t_host = min(a.host_objects, shape["N"]), min(a.host_samples, T)
        part = {k: (v[:t_host] if k in SAMPLES else v) for k, v in case.items()}
        part.update(codes=case["codes"][:n_host], groups=case["groups"][:, :n_host], clusters=np.ascontiguousarray(case["clusters"][:t_host, :, :n_host]))
        seconds, _ = wall(lambda: orc.run(**part))
        scale = shape["N"] / n_host * T / t_host
        run["host"] = {"checker_objects": n_host, "checker_samples": t_host, "checker_s": round(seconds / 1e3, 3),
                       "checker_s_scaled_to_the_shape": round(seconds / 1e3 * scale, 2)}
        out["runs"].append(run)
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
