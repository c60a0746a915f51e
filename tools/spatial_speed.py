"""Speed of sbayes_amd.spatial at the two shapes of tools/ppc_speed.py (1000 objects x 200 features x 10 states; the
south_america shape, 100 x 36 x 5), T = 1000 replicates each, once with one class over a symmetrised 6-nearest-neighbour graph
("knn6") and once with 8 quantile classes over all pairs ("bands8"); prints one JSON line and writes it to --out.

The replicates are those of the posterior predictive check of a seeded case (sbayes_amd.ppc, whose own check with the replicates
copied back is timed in the same session: "ppc_check"); the objects are seeded points in the unit square.  Device: 2 warm-up and
5 timed repeats of add() on all replicates: the unit's kernels by HIP events (summed over the library calls the block was split
into) and the wall time of the synchronous call, smallest and median; set_data once.  Host: the NumPy checker
(tests/_spatial_oracle.py) over --host-replicates replicates on the same host, its seconds per replicate and that figure SCALED
to T (it is not run on all of them), with whether the device's arrays of those replicates equal the checker's.
    python tools/spatial_speed.py [--replicates 1000] [--out profiles/spatial/spatial_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import ppc, spatial                  # noqa: E402
from tests import _predict_oracle as predict_orc     # noqa: E402
from tests import _spatial_oracle as orc             # noqa: E402

SHAPES = {"headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10]),
          "south_america": dict(N=100, F=36, S=5, C=3, K=3, group_counts=[1, 6])}
CLASSES = {"knn6": dict(knn=6), "bands8": dict(n_bands=8)}
WARMUP, REPEATS = 2, 5
SEED = 2901


def summary(walls, kernels, calls):
    return {"kernel_ms": round(min(kernels), 4), "kernel_ms_median": round(float(np.median(kernels)), 4), "call_ms": round(min(walls), 4),
            "call_ms_median": round(float(np.median(walls)), 4), "library_calls": calls, "warmup": WARMUP, "repeats": REPEATS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, default=2)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "spatial" / "spatial_speed.json")
    a = ap.parse_args()
    out = {"tool": "spatial_speed", "replicates": a.replicates, "seed": SEED, "runs": []}
    hp, h = ppc.PpcHandle(0), spatial.SpatialHandle(0)
    for name, shape in SHAPES.items():
        case = predict_orc.random_case(1, T=a.replicates, out_share=0.2, na_share=0.05, **shape)
        hp.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        walls, kernels = [], []
        for i in range(WARMUP + REPEATS):
            hp.reset()
            t0 = time.perf_counter()
            hp.check(case["clusters"], case["weights"], case["tables"], seed=SEED, replicates=True)
            if i >= WARMUP:
                walls.append((time.perf_counter() - t0) * 1e3)
                kernels.append(hp.kernel_ms)
        ppc_check = summary(walls, kernels, -(-a.replicates // hp.max_samples(True)))
        y = hp.result().y_rep
        n_states = np.full(shape["F"], shape["S"], dtype=np.int32)
        costs = spatial.plane_distances(np.random.default_rng(SEED).random((shape["N"], 2)))
        for classes, how in CLASSES.items():
            band, b = spatial.bands_from_costs(costs, **how)
            t0 = time.perf_counter()
            h.set_data(case["codes"], n_states, band, b)
            run = {"shape": name, "classes": classes, "B": b, **{k: v for k, v in shape.items() if k in "NFS"},
                   "counted_pairs": int((band != spatial.NA).sum()) // 2, "set_data_ms": round((time.perf_counter() - t0) * 1e3, 3),
                   "observed_kernel_ms": round(h.last_kernel_ms(), 4), "replicates_per_library_call": h.call_replicates()}
            walls, kernels = [], []
            for i in range(WARMUP + REPEATS):
                h.reset()
                t0 = time.perf_counter()
                h.add(y)
                if i >= WARMUP:
                    walls.append((time.perf_counter() - t0) * 1e3)
                    kernels.append(h.kernel_ms)
            run["add"] = summary(walls, kernels, -(-a.replicates // h.call_replicates()))
            run["ppc_check"] = ppc_check
            res = h.result()
            run["p_total"] = [float(v) for v in res.p_value("total")]
            th = min(a.host_replicates, a.replicates)
            t0 = time.perf_counter()
            want = [orc.statistics(y[t], band, b) for t in range(th)]
            seconds = (time.perf_counter() - t0) / th
            h.reset()
            h.add(y[:th], keep=True)
            got = h.result()
            equal = all(np.array_equal(getattr(got, f"{k}_rep")[t], want[t][k]) for t in range(th) for k in orc.STATS)
            run["host"] = {"oracle_replicates": th, "oracle_s_per_replicate": round(seconds, 6), "oracle_s_scaled_to_replicates": round(seconds * a.replicates, 3),
                           "scaled": True, "device_equals_oracle": bool(equal),
                           "device_call_faster_than_scaled_oracle": bool(run["add"]["call_ms"] < seconds * a.replicates * 1e3)}
            out["runs"].append(run)
    h.close()
    hp.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
