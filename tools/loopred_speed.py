"""Speed of sbayes_amd.loopred at the south_america shape (100 objects x 36 features x 5 states, two confounders of 1 and 6 groups)
and at the headline shape (1000 x 200 x 10, one confounder of 10 groups), K = 5 clusters and T = 1000 samples each; prints one JSON
line and writes it to --out.

Per shape, in one process, 1 warm-up and 3 timed repeats of each, the variants of one repeat run one after the other (alternating):
  loopred      the three phases from an empty store: add, weights, accumulate, then the read: the kernels' time by HIP events,
               summed over the library calls a pass was split into, and the wall time of the synchronous calls;
  the existing route to loo_i alone: predict.accumulate with the lik rows copied back, elpd's append_rows, elpd's compute;
  predict's plain accumulate (no lik), which phase 3 is reported against: it adds 8 + 4 bytes and S multiplies per (cell, sample).
Smallest and median of the repeats.  Host: the NumPy oracle (tests/_loopred_oracle.py) over the first --host-objects objects and
all samples, scaled to the N objects.
    python tools/loopred_speed.py [--samples 1000] [--out profiles/loopred/loopred_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import elpd, loopred, predict       # noqa: E402
from tests import _loopred_oracle as orc            # noqa: E402
from tests import _predict_oracle as po             # noqa: E402

SHAPES = {"south_america": dict(N=100, F=36, S=5, C=3, K=5, group_counts=[1, 6]),
          "headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10])}
WARMUP, REPEATS = 1, 3
SAMPLES = ("clusters", "weights", "tables")


def make_case(shape, T):
    """A seeded case whose observed cells have a positive likelihood in every sample: every object is in a group of the first
    confounder (a fifth of them are in no cluster of a sample)."""
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
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "loopred" / "loopred_speed.json")
    a = ap.parse_args()
    T = a.samples
    out = {"tool": "loopred_speed", "samples": T, "warmup": WARMUP, "repeats": REPEATS, "runs": []}
    for name, shape in SHAPES.items():
        case = make_case(shape, T)
        samples = tuple(case[k] for k in SAMPLES)
        na = (case["codes"] == po.NA).ravel()
        M = int((~na).sum())
        h = loopred.LooPredHandle(0)
        p = predict.PredictHandle(0)
        store = elpd._Store(0, na.size, T)
        h.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"], capacity=T)
        p.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        times = {k: [] for k in ("add_call", "add_kernel", "weights_call", "weights_kernel", "accumulate_call", "accumulate_kernel", "read_call",
                                 "route_predict_lik_call", "route_predict_lik_kernel", "route_append_call", "route_compute_call", "route_compute_kernel", "predict_plain_call", "predict_plain_kernel")}
        results = {}
        for i in range(WARMUP + REPEATS):
            rec = {}
            h.reset()
            rec["add_call"], _ = wall(lambda: h.add(*samples))
            rec["add_kernel"] = h.kernel_ms["add"]
            rec["weights_call"], pointwise = wall(h.weights)
            rec["weights_kernel"] = h.kernel_ms["weights"]
            rec["accumulate_call"], _ = wall(lambda: h.accumulate(*samples))
            rec["accumulate_kernel"] = h.kernel_ms["accumulate"]
            rec["read_call"], (p_loo, n_done) = wall(h.sums)
            # the existing route to loo_i
            p.reset()
            store.reset()
            rec["route_predict_lik_call"], lik = wall(lambda: p.accumulate(*samples, lik=True))
            rec["route_predict_lik_kernel"] = p.kernel_ms
            rec["route_append_call"], _ = wall(lambda: store.append_rows(lik))
            rec["route_compute_call"], (loo_i, k_i, _lppd, _v) = wall(lambda: store.compute(0, na, False))
            rec["route_compute_kernel"] = store.last_kernel_ms()
            p.reset()
            rec["predict_plain_call"], _ = wall(lambda: p.accumulate(*samples))
            rec["predict_plain_kernel"] = p.kernel_ms
            if i >= WARMUP:
                for k, v in rec.items():
                    times[k].append(v)
            results = dict(p_loo=p_loo, loo=(pointwise[0].copy(), pointwise[1].copy()), route=(loo_i, k_i))
            del lik
        assert n_done == T and np.isfinite(results["p_loo"]).all()
        assert np.array_equal(results["loo"][0], results["route"][0]) and np.array_equal(results["loo"][1], results["route"][1], equal_nan=True)
        run = {"shape": name, **{k: v for k, v in shape.items() if k != "group_counts"}, "R": shape["K"] + sum(shape["group_counts"]), "observed_cells": M,
               "store_bytes": loopred.store_bytes(M, T), "library_calls_per_pass": -(-T // h.max_samples()),
               "lik_bytes_each_way_existing_route": 4 * na.size * T, "ms": {k: stats(v) for k, v in times.items()},
               "same_bits": {"loo_i_and_k_as_the_existing_route": True},
               "n_bad_k": int((~(results["loo"][1] <= 0.7)).sum())}
        ms = run["ms"]
        run["phases_1_and_2_call_ms"] = round(ms["add_call"]["min"] + ms["weights_call"]["min"], 4)
        run["existing_route_call_ms"] = round(ms["route_predict_lik_call"]["min"] + ms["route_append_call"]["min"] + ms["route_compute_call"]["min"], 4)
        h.close()
        p.close()
        store.close()
        n_host = min(a.host_objects, shape["N"])
        part = {k: v for k, v in case.items()}
        part.update(codes=case["codes"][:n_host], groups=case["groups"][:, :n_host], clusters=np.ascontiguousarray(case["clusters"][:, :, :n_host]))
        seconds, _ = wall(lambda: orc.run(**part))
        run["host"] = {"oracle_objects": n_host, "oracle_s": round(seconds / 1e3, 3), "oracle_s_scaled_to_objects": round(seconds / 1e3 * shape["N"] / n_host, 2)}
        out["runs"].append(run)
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
