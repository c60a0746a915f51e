"""Speed of the posterior summary (sbayes_amd.summary) at the widths of a stats file -- P = 12 400 columns at 5 runs x 2000
samples and at 5 x 10 000 -- with, in the same run on the same rows: the diagnostics' column kernel alone
(sbayes_amd.diag, sbe_diag_compute), and the NumPy restatement with direct sums (tests/_summary_oracle.py, exact=False) on 200 columns of the same host;
prints one JSON line and writes it to --out.

Columns are AR(1) with phi spread over [0, 0.99].  Device: the rank kernel's and the column passes' time by HIP events
(SummaryResult.rank_ms, column_ms) and the wall time of the whole call with upload.  The summary runs the column kernel
five times (the store and four derived columns) and sorts twice, so about five times the diagnostics' kernel is expected.
    python tools/summary_speed.py [--shapes 12400x5x2000 12400x5x10000] [--out profiles/summary/summary_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import diag, summary             # noqa: E402
from tests import _diag_oracle as orc            # noqa: E402
from tests import _summary_oracle as sorc        # noqa: E402


def one_shape(hs, hd, p, m, s, oracle_columns, repeats):
    rng = np.random.default_rng(p + s)
    phi = np.linspace(0.0, 0.99, p)
    rng.shuffle(phi)
    chains = [orc.ar1(rng, phi, 1, s, p)[0] for _ in range(m)]
    head = [x[:, :oracle_columns].copy() for x in chains]
    walls, rank_ms, column_ms, diag_ms, res = [], [], [], [], None
    for _ in range(repeats + 1):                      # (the first pass warms the runtime and sizes the buffers)
        t0 = time.perf_counter()
        hs.reset(m, p, s)
        for c in range(m):
            hs.append(c, chains[c])
        res = hs.compute(burnin=0.1)
        walls.append(time.perf_counter() - t0)
        rank_ms.append(res.rank_ms)
        column_ms.append(res.column_ms)
        hd.reset(m, p, s)
        for c in range(m):
            hd.append(c, chains[c])
        ref = hd.compute(burnin=0.1)
        diag_ms.append(ref.kernel_ms)
    same = all(getattr(res, k).tobytes() == getattr(ref, k).tobytes() for k in ("mean", "sd", "ess", "rhat", "mcse_mean", "n_lags"))
    del chains
    t0 = time.perf_counter()
    want = sorc.summarize(head, burnin=0.1, exact=False)
    host = (time.perf_counter() - t0) * p / oracle_columns
    agree = int(np.sum(np.isclose(res.ess_bulk[:oracle_columns], want["ess_bulk"], rtol=1e-8)
                       & np.isclose(res.ess_tail[:oracle_columns], want["ess_tail"], rtol=1e-8)
                       & (res.quantiles[:, :oracle_columns] == want["quantiles"]).all(axis=0)))
    rank, column, dg = min(rank_ms[1:]), min(column_ms[1:]), min(diag_ms[1:])
    return {"columns": p, "runs": m, "samples": s, "chains": res.n_chains, "draws": res.n_draws, "path": res.path,
            "launches": res.launches, "launch_columns": res.launch_columns, "rank_kernel_ms": round(rank, 3),
            "column_passes_ms": round(column, 3), "diag_kernel_ms": round(dg, 3), "ratio_to_diag_kernel": round((rank + column) / dg, 2),
            "upload_and_compute_ms": round(min(walls[1:]) * 1e3, 3), "first_call_ms": round(walls[0] * 1e3, 3),
            "numpy_checker_s_scaled": round(host, 2), "numpy_checker_ms_per_column": round(host / p * 1e3, 4),
            "speedup_kernels": round(host / ((rank + column) / 1e3), 1), "diag_outputs_bit_equal": bool(same),
            "ess_bulk_median": round(float(np.median(res.ess_bulk)), 1), "ess_tail_median": round(float(np.median(res.ess_tail)), 1),
            "host_columns": oracle_columns, "host_columns_agreeing": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["12400x5x2000", "12400x5x10000"], help="columns x runs x samples")
    ap.add_argument("--oracle-columns", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default="profiles/summary/summary_speed.json")
    a = ap.parse_args()
    out = {"tool": "summary_speed", "lds_max_draws": summary.lds_max_draws(), "shapes": []}
    hs, hd = summary.SummaryHandle(0), diag.DiagHandle(0)
    try:
        for shape in a.shapes:
            p, m, s = (int(v) for v in shape.split("x"))
            out["shapes"].append(one_shape(hs, hd, p, m, s, min(a.oracle_columns, p), a.repeats))
            print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)
    finally:
        hs.close()
        hd.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
