"""Speed of sbayes_amd.ppc at the two shapes of tools/predict_speed.py (1000 objects x 200 features x 10 states, K = 5 clusters
and one confounder of 10 groups; the south_america shape, 100 x 36 x 5, K = 3, two confounders of 1 and 6 groups), T = 1000
samples each; prints one JSON line and writes it to --out.

Device: 2 warm-up and 5 timed repeats of check() on all samples, without and with the replicates copied back: the kernels' time
by HIP events (preparation, validation, draws and sums, summed over the library calls the block was split into) and the wall
time of the synchronous call, smallest and median; the upload (set_data) once.  Next to them, in the same session, the
posterior predictive's accumulate call at the same shape (sbayes_amd.predict, without the lik rows), so that a reader sees what
the draw, the two logs and the sums cost, and the NumPy oracle (tests/_ppc_oracle.py) over --host-samples samples on the same
host, with its seconds per sample and scaled to T.
    python tools/ppc_speed.py [--samples 1000] [--out profiles/ppc/ppc_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import ppc, predict                  # noqa: E402
from tests import _ppc_oracle as orc                 # noqa: E402
from tests import _predict_oracle as predict_orc     # noqa: E402

SHAPES = {"headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10]),
          "south_america": dict(N=100, F=36, S=5, C=3, K=3, group_counts=[1, 6])}
WARMUP, REPEATS = 2, 5
SEED = 2201


def summary(walls, kernels, calls):
    return {"kernel_ms": round(min(kernels), 4), "kernel_ms_median": round(float(np.median(kernels)), 4), "call_ms": round(min(walls), 4),
            "call_ms_median": round(float(np.median(walls)), 4), "library_calls": calls, "warmup": WARMUP, "repeats": REPEATS}


def timed_check(h, case, replicates):
    walls, kernels = [], []
    for i in range(WARMUP + REPEATS):
        h.reset()
        t0 = time.perf_counter()
        h.check(case["clusters"], case["weights"], case["tables"], seed=SEED, replicates=replicates)
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(h.kernel_ms)
    return summary(walls, kernels, -(-case["clusters"].shape[0] // h.max_samples(replicates)))


def timed_accumulate(h, case):
    walls, kernels = [], []
    for i in range(WARMUP + REPEATS):
        h.reset()
        t0 = time.perf_counter()
        h.accumulate(case["clusters"], case["weights"], case["tables"])
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(h.kernel_ms)
    return summary(walls, kernels, -(-case["clusters"].shape[0] // h.max_samples()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--host-samples", type=int, default=10)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "ppc" / "ppc_speed.json")
    a = ap.parse_args()
    out = {"tool": "ppc_speed", "samples": a.samples, "seed": SEED, "runs": []}
    h, hp = ppc.PpcHandle(0), predict.PredictHandle(0)
    for name, shape in SHAPES.items():
        case = predict_orc.random_case(1, T=a.samples, out_share=0.2, na_share=0.05, **shape)
        t0 = time.perf_counter()
        h.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        run = {"shape": name, **{k: v for k, v in shape.items() if k != "group_counts"}, "R": shape["K"] + sum(shape["group_counts"]),
               "upload_ms": round((time.perf_counter() - t0) * 1e3, 3)}
        run["without_replicates"] = timed_check(h, case, False)
        run["with_replicates"] = timed_check(h, case, True)
        res = h.result()
        run["n_samples"], run["n_skipped"], run["p_total"] = res.n_samples, res.n_skipped, res.p_total
        hp.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        run["predict_accumulate"] = timed_accumulate(hp, case)
        th = min(a.host_samples, a.samples)
        part = {k: (v[:th] if k in ("clusters", "weights", "tables") else v) for k, v in case.items()}
        t0 = time.perf_counter()
        want = orc.check(seed=SEED, **part)
        seconds = time.perf_counter() - t0
        run["host"] = {"oracle_samples": th, "oracle_s_per_sample": round(seconds / th, 6), "oracle_s_scaled_to_samples": round(seconds / th * a.samples, 3),
                       "replicate_equals_oracle": bool(np.array_equal(res.y_rep[:th], want["y_rep"])),
                       "smallest_margin": float(want["margin"][want["drawn"]].min())}
        out["runs"].append(run)
    h.close()
    hp.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
