"""Speed of the power-scaling sensitivity (sbayes_amd.psens) at the size of a real run -- P = 10 000 columns x N = 10 000 draws x
G = 6 components -- and at the shape of the recorded small runs (tests/golden/diag_runs.npz), with, in the same session on the
same rows: the summary's rank kernel (sbayes_amd.summary: two sorts per column and the ranks; the yardstick for "a sort per
column") and the NumPy checker (tests/_psens_oracle.py) on 32 columns of the same host, scaled.  Also measures the error of the
device's float64 log2 against mpmath on (i + 1) / 1000, the figure the tests' bound on js takes its L from.  Prints one JSON line
and writes it to --out.

Device times are HIP events around the kernels (last_kernel_times); call times are a host clock around calls that end in a
synchronise; the first pass of every shape warms the runtime and sizes the buffers and is reported apart.
    python tools/psens_speed.py [--shapes 10000x1x10000 golden] [--out profiles/psens/psens_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from sbayes_amd import psens, summary            # noqa: E402
from tests import _psens_oracle as orc           # noqa: E402

COMPONENTS = 6


def log2_error(h, n=1000):
    """The device's log2 on (i + 1) / n against 50 digits, in ulps of the exact value's binade."""
    import mpmath
    x = np.arange(1, n + 1, dtype=np.float64) / n
    got = h.device_log2(x)
    host = np.log2(x)
    worst = worst_host = 0.0
    with mpmath.workdps(50):
        for xi, gi, hi in zip(x, got, host):
            exact = mpmath.log(mpmath.mpf(float(xi))) / mpmath.log(2)
            if exact == 0:
                assert gi == 0.0
                continue
            ulp = mpmath.mpf(float(np.spacing(abs(float(exact)))))
            worst = max(worst, float(abs(mpmath.mpf(float(gi)) - exact) / ulp))
            worst_host = max(worst_host, float(abs(mpmath.mpf(float(hi)) - exact) / ulp))
    return {"values": n, "device_log2_max_ulp": round(worst, 4), "numpy_log2_max_ulp": round(worst_host, 4),
            "device_equals_numpy": int(np.sum(got == host))}


def synthetic(p, m, s):
    """m runs of s rows: the first COMPONENTS columns are log densities -z^2 / 2 at growing scales, the rest normal draws, a
    tenth of them rounded to integers (ties)."""
    rng = np.random.default_rng(p + s)
    runs = []
    for _ in range(m):
        x = rng.standard_normal((s, p))
        x[:, :COMPONENTS] = -0.5 * x[:, :COMPONENTS] ** 2 * (10.0 * (1 + np.arange(COMPONENTS)))
        x[:, COMPONENTS::10] = np.round(x[:, COMPONENTS::10] * 3.0)
        runs.append(x)
    return [f"c{j}" for j in range(p)], runs, list(range(COMPONENTS))


def golden():
    g = np.load(REPO / "tests" / "golden" / "diag_runs.npz")
    names = [str(v) for v in g["names"]]
    return names, [np.ascontiguousarray(g["stats_0"]), np.ascontiguousarray(g["stats_1"])], [names.index(c) for c in psens.DEFAULT_COMPONENTS]


def one_shape(hp, hs, label, names, runs, columns, oracle_columns, repeats, delta=0.01, burnin=0.1):
    m, p, s = len(runs), runs[0].shape[1], max(len(r) for r in runs)
    upload, weights_call, column_call, weights_ms, column_ms, rank_ms, sums = [], [], [], [], [], [], None
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        hp.reset(m, p, s)
        for c in range(m):
            hp.append(c, runs[c])
        t1 = time.perf_counter()
        k, ess, vflag = hp.weights_from_components(columns, delta=delta, burnin=burnin)
        t2 = time.perf_counter()
        sums = hp.compute()
        t3 = time.perf_counter()
        upload.append(t1 - t0)
        weights_call.append(t2 - t1)
        column_call.append(t3 - t2)
        wm, cm = hp.last_kernel_times()
        weights_ms.append(wm)
        column_ms.append(cm)
    chains, n, v, path, launches, per_launch = hp.last_shape()
    hp.reset(1, 1, 1)                                                        # (the store's memory stays with the handle; the summary gets its own)
    for _ in range(2):
        hs.reset(m, p, s)
        for c in range(m):
            hs.append(c, runs[c])
        rank_ms.append(hs.compute(burnin=burnin, split=False).rank_ms)
    stacked = orc.stack([r[:, list(columns) + list(range(oracle_columns))] for r in runs], [int(burnin * len(r)) for r in runs])
    t0 = time.perf_counter()
    lws, ks, _ess, flags = orc.component_weights(stacked, list(range(len(columns))), delta)
    t1 = time.perf_counter()
    weights = np.where((flags & orc.VFLAG_CONSTANT)[:, None] != 0, 1.0 / len(stacked), np.exp(lws))
    want = orc.table(stacked[:, len(columns):], weights, flags)
    host_columns = time.perf_counter() - t1
    agree = int(np.sum(np.all(np.abs(sums.js[:, :oracle_columns] - want["js"]) <= orc.bound_js(n, want["magnitude"]) + 1.6e-9 * want["magnitude"], axis=0)))
    col, rank = min(column_ms[1:]), min(rank_ms[1:])
    cjs = sums.cjs()
    return {"shape": label, "columns": p, "runs": m, "rows": s, "draws": n, "vectors": v, "path": path, "launches": launches,
            "launch_columns": per_launch, "upload_ms": round(min(upload[1:]) * 1e3, 3), "weights_kernel_ms": round(min(weights_ms[1:]), 3),
            "weights_call_ms": round(min(weights_call[1:]) * 1e3, 3), "column_kernel_ms": round(col, 3),
            "column_call_ms": round(min(column_call[1:]) * 1e3, 3), "first_pass_ms": round((upload[0] + weights_call[0] + column_call[0]) * 1e3, 3),
            "column_kernel_ms_all_passes": [round(c, 3) for c in column_ms], "summary_rank_kernel_ms": round(rank, 3),
            "column_kernel_over_rank_kernel": round(col / rank, 2), "log2_per_second": round(6.0 * v * n * p / (col / 1e3), 0),
            "numpy_checker_weights_s": round(t1 - t0, 3), "numpy_checker_columns_s_scaled": round(host_columns * p / oracle_columns, 2),
            "speedup_column_kernel": round(host_columns * p / oracle_columns / (col / 1e3), 1), "host_columns": oracle_columns,
            "host_columns_agreeing": agree, "pareto_k": [round(float(x), 3) for x in k], "vflag": [int(x) for x in vflag],
            "cjs_median": round(float(np.nanmedian(cjs)), 6), "cjs_max": round(float(np.nanmax(cjs)), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000x1x10000", "golden"], help="columns x runs x rows, or `golden`")
    ap.add_argument("--oracle-columns", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default="profiles/psens/psens_speed.json")
    a = ap.parse_args()
    out = {"tool": "psens_speed", "lds_max_draws": psens.lds_max_draws(), "shapes": []}
    hp, hs = psens.PsensHandle(0), summary.SummaryHandle(0)
    try:
        out["log2"] = log2_error(hp)
        print(json.dumps(out["log2"]), file=sys.stderr, flush=True)
        for shape in a.shapes:
            if shape == "golden":
                names, runs, columns = golden()
            else:
                p, m, s = (int(v) for v in shape.split("x"))
                names, runs, columns = synthetic(p, m, s)
            out["shapes"].append(one_shape(hp, hs, shape, names, runs, columns, min(a.oracle_columns, runs[0].shape[1]), a.repeats))
            print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)
            del runs
    finally:
        hp.close()
        hs.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
