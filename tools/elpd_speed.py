"""Speed of sbayes_amd.elpd.psis_loo at the headline width (M = 200 000 observations) against the NumPy restatement
(tests/_elpd_oracle.py) on the same host; prints one JSON line.

Device: the column kernel's time by HIP events (the store's last compute call), the synchronous compute call's wall
time, and the wall time of the whole host path (upload of the float32 matrix + compute); achieved GB/s on S*M*4
bytes.  Host: the restatement on 200 columns, scaled to M.
    python tools/elpd_speed.py [--m 200000] [--samples 1000 10000] [--oracle-columns 200]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import elpd                      # noqa: E402
from tests import _elpd_oracle as eo             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200_000)
    ap.add_argument("--samples", type=int, nargs="+", default=[1000, 10_000])
    ap.add_argument("--oracle-columns", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"tool": "elpd_speed", "m": a.m, "lds_max_samples": elpd.lds_max_samples(), "runs": []}
    rng = np.random.default_rng(0)
    for s in a.samples:
        lh = rng.standard_normal((s, a.m), dtype=np.float32)          # (float32 throughout: 8 GB at S = 10 000)
        lh *= 0.8
        lh -= 1.5
        np.exp(lh, out=lh)
        na = np.zeros(a.m, bool)
        t0 = time.perf_counter()
        res = elpd.psis_loo(lh, na_values=na, burnin=0.0)                 # (first call: also warms the runtime)
        first = time.perf_counter() - t0
        walls = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            elpd.psis_loo(lh, na_values=na, burnin=0.0)
            walls.append(time.perf_counter() - t0)
        st = elpd._Store(0, a.m, s)
        st.append_rows(lh)
        calls, kernels = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            st.compute(0, na, False)
            calls.append(time.perf_counter() - t0)
            kernels.append(st.last_kernel_ms())
        st.close()
        cols = a.oracle_columns
        t0 = time.perf_counter()
        want = np.array([eo.column_stats(lh[:, j]) for j in range(cols)])
        host = (time.perf_counter() - t0) * a.m / cols
        assert np.allclose(res.loo_i[:cols], want[:, 0], rtol=1e-10, atol=1e-10)
        kern = min(kernels) / 1e3
        out["runs"].append({
            "samples": s, "bytes": s * a.m * 4, "kernel_ms": round(min(kernels), 3), "compute_call_ms": round(min(calls) * 1e3, 3),
            "upload_and_compute_ms": round(min(walls) * 1e3, 3), "first_call_ms": round(first * 1e3, 3),
            "kernel_gb_s": round(s * a.m * 4 / kern / 1e9, 1), "oracle_s_scaled": round(host, 2),
            "speedup_kernel": round(host / kern, 1), "speedup_upload_and_compute": round(host / min(walls), 1)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
