"""Speed of sbayes_amd.compare at the headline sizes (N = 200 000 observations with M = 7 models, N = 1 000 000 with M = 8;
B = 1000 bootstrap replicates) against the host recipes on the same machine; prints one JSON line and writes it to --out.

Device, per call (totals, differences, stacking, bootstrap): the first call on the new store (it loads code objects and
allocates; the first stacking call also builds the p image, which every one-shot compare() pays), then over --repeats further
calls the kernels' time by HIP events (last_kernel_ms; for stacking the span holds the host's reads of the gap) and the wall
time of the synchronous call: smallest, median and largest; the stacking update count, the time per update and the objective
reached.  Host: the restatement's EM (tests/_compare_oracle.py, NumPy sums) run to the same tolerance, with its seconds,
updates, gap and objective, arviz's SLSQP recipe with the objective it reaches, and arviz's bootstrap recipe in NumPy
(Dirichlet draws [B, N], then a Python loop over the replicates) at B = 1000 where the 1.6 GB matrix fits and at the reduced
B recorded beside it where it does not.
    python tools/compare_speed.py [--shapes 200000x7 1000000x8] [--b 1000] [--out profiles/compare/compare_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import compare                      # noqa: E402
from tests import _compare_oracle as co             # noqa: E402

HOST_DRAW_BYTES = 2 << 30                           # the host recipe's Dirichlet matrix is kept under 2 GiB


def timed(call, repeats, handle):
    t0 = time.perf_counter()
    call()                                          # the first call: code objects, allocations, for stacking the p image
    first = time.perf_counter() - t0
    first_kernel = handle.last_kernel_ms()
    walls, kernels, result = [], [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        result = call()
        walls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(handle.last_kernel_ms())
    return result, {"kernel_ms": round(min(kernels), 4), "call_ms": round(min(walls), 4),
                    "kernel_ms_median": round(float(np.median(kernels)), 4), "kernel_ms_max": round(max(kernels), 4),
                    "call_ms_median": round(float(np.median(walls)), 4), "call_ms_max": round(max(walls), 4), "repeats": repeats,
                    "first_call_ms": round(first * 1e3, 4), "first_kernel_ms": round(first_kernel, 4)}


def host_bootstrap(x, b, seed):
    """arviz's BB-pseudo-BMA recipe in NumPy: (weights, seconds)."""
    n, m = x.shape
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    draws = rng.dirichlet(np.ones(n), size=b)       # [b, n]
    z = (draws @ x) * n
    weights = np.zeros(m)
    for row in z:                                   # (arviz loops over the replicates in Python)
        t = np.exp(row - row.max())
        weights += t / t.sum()
    return weights / b, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["200000x7", "1000000x8"])
    ap.add_argument("--b", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "compare" / "compare_speed.json")
    a = ap.parse_args()
    out = {"tool": "compare_speed", "b": a.b, "tol": a.tol, "check_every": compare.CHECK_EVERY, "chunk": compare.CHUNK, "boot_chunk": compare.BOOT_CHUNK,
           "runs": []}
    h = compare.CompareHandle(0)
    for shape in a.shapes:
        n, m = (int(v) for v in shape.split("x"))
        x = co.gamma_values(1, n, m)
        t0 = time.perf_counter()
        h.reset(m, n)
        for k in range(m):
            h.set_model(k, x[:, k])
        run = {"n": n, "m": m, "upload_ms": round((time.perf_counter() - t0) * 1e3, 3)}
        (elpd, _se), run["totals"] = timed(h.totals, a.repeats, h)
        _, run["differences"] = timed(lambda: h.differences(int(np.argmax(elpd))), a.repeats, h)
        (w, gap, updates, converged), run["stacking"] = timed(lambda: h.stacking(a.tol), a.repeats, h)
        run["stacking"].update(updates=updates, gap=gap, converged=bool(converged), objective=co.objective(x, w),
                               us_per_update=round(run["stacking"]["kernel_ms"] * 1e3 / max(updates + 1, 1), 3))
        (bw, _bse), run["bootstrap"] = timed(lambda: h.bootstrap(0, a.b), a.repeats, h)
        run["bootstrap"]["draws_per_s"] = round(a.b * n / (run["bootstrap"]["kernel_ms"] / 1e3), 1)
        # ---- the host recipes ----
        t0 = time.perf_counter()
        w_host, gap_host, updates_host, converged_host = co.stacking(x, tol=a.tol, exact=False)
        seconds = time.perf_counter() - t0
        host = {"em_s": round(seconds, 3), "em_updates": updates_host, "em_gap": gap_host, "em_converged": bool(converged_host),
                "em_objective": co.objective(x, w_host), "em_ms_per_update": round(seconds * 1e3 / (updates_host + 1), 3)}
        t0 = time.perf_counter()
        w_slsqp = co.stacking_slsqp(x)
        host.update(slsqp_s=round(time.perf_counter() - t0, 3), slsqp_objective=co.objective(x, w_slsqp),
                    slsqp_returned_its_start=bool(np.allclose(w_slsqp, 1.0 / m, rtol=0, atol=1e-12)))
        b_host = max(1, min(a.b, HOST_DRAW_BYTES // (8 * n)))
        w_boot, seconds = host_bootstrap(x, b_host, 0)
        host.update(bootstrap_b=b_host, bootstrap_s=round(seconds, 3), bootstrap_s_scaled_to_b=round(seconds * a.b / b_host, 3),
                    bootstrap_max_weight_difference=float(np.max(np.abs(w_boot - bw))))      # (other draws: agreement in distribution only)
        run["host"] = host
        out["runs"].append(run)
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
