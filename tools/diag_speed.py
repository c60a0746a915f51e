"""Speed of the convergence diagnostics (sbayes_amd.diag) at the widths of a stats file -- P = 12 400 columns (headline)
and 510 000 (stress) at 5 runs x 2000 samples, and P = 12 400 at 5 x 10 000 -- against the NumPy restatement with direct
sums (tests/_diag_oracle.py, exact=False) on the same host in the same run; prints one JSON line and writes it to --out.

Columns are AR(1) with phi spread over [0, 0.99].  Device: the column kernel's time by HIP events (last_kernel_ms), and
the wall time of the whole call with upload (reset, the appends of every run, compute).  Host: the restatement on 200
columns, scaled to P.  --worst adds a launch whose columns all run to the n - 3 bound of the positive sequence (runs
shifted against each other), the case the launch rule of DESIGN.md section 16 is sized for.
    python tools/diag_speed.py [--shapes 12400x5x2000 510000x5x2000 12400x5x10000] [--worst] [--out profiles/diag/diag_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import diag                      # noqa: E402
from tests import _diag_oracle as orc            # noqa: E402


def one_shape(h, p, m, s, oracle_columns, repeats, shift=0.0):
    rng = np.random.default_rng(p + s)
    phi = np.linspace(0.0, 0.99, p)
    rng.shuffle(phi)
    head = []
    t_gen = time.perf_counter()
    chains = []
    for c in range(m):                                # (one run at a time: 8 GB each at the stress width)
        x = orc.ar1(rng, phi, 1, s, p)[0]
        if shift:
            x += shift * c
        chains.append(x)
        head.append(x[:, :oracle_columns].copy())
    t_gen = time.perf_counter() - t_gen
    walls, kernels, res = [], [], None
    for _ in range(repeats + 1):                      # (the first pass warms the runtime and sizes the buffers)
        t0 = time.perf_counter()
        h.reset(m, p, s)
        for c in range(m):
            h.append(c, chains[c])
        res = h.compute(burnin=0.1)
        walls.append(time.perf_counter() - t0)
        kernels.append(res.kernel_ms)
    del chains
    t0 = time.perf_counter()
    x, _cut = orc.prepare(head, 0.1, True)
    want = [orc.column(np.ascontiguousarray(x[:, :, j]), exact=False) for j in range(oracle_columns)]
    host = (time.perf_counter() - t0) * p / oracle_columns
    agree = int(np.sum(np.isclose(res.ess[:oracle_columns], [w["ess"] for w in want], rtol=1e-8)
                       & (res.n_lags[:oracle_columns] == [w["n_lags"] for w in want])))
    kern = min(kernels[1:]) / 1e3
    wall = min(walls[1:])
    return {"columns": p, "runs": m, "samples": s, "chains": res.n_chains, "draws": res.n_draws, "path": res.path,
            "launches": res.launches, "bytes": p * m * s * 8, "kernel_ms": round(kern * 1e3, 3),
            "upload_and_compute_ms": round(wall * 1e3, 3), "first_call_ms": round(walls[0] * 1e3, 3),
            "numpy_direct_s_scaled": round(host, 2), "numpy_direct_ms_per_column": round(host / p * 1e3, 4),
            "speedup_kernel": round(host / kern, 1), "speedup_upload_and_compute": round(host / wall, 1),
            "n_lags_mean": round(float(res.n_lags.mean()), 1), "n_lags_max": int(res.n_lags.max()),
            "ess_median": round(float(np.median(res.ess)), 1), "host_columns": oracle_columns, "host_columns_agreeing": agree, "generate_s": round(t_gen, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["12400x5x2000", "510000x5x2000", "12400x5x10000"], help="columns x runs x samples")
    ap.add_argument("--oracle-columns", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"tool": "diag_speed", "lds_max_draws": diag.lds_max_draws(), "shapes": []}
    h = diag.DiagHandle(0)
    try:
        for shape in a.shapes:
            p, m, s = (int(v) for v in shape.split("x"))
            out["shapes"].append(one_shape(h, p, m, s, min(a.oracle_columns, p), a.repeats))
            print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)
        if a.worst:
            w = one_shape(h, 12400, 5, 2000, 8, 1, shift=3.0)
            w["multiply_adds"] = w["columns"] * w["chains"] * w["draws"] ** 2 // 2
            w["multiply_adds_per_s"] = round(w["multiply_adds"] / (w["kernel_ms"] / 1e3), 1)
            out["worst_case"] = w
    finally:
        h.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
