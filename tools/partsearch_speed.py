"""Speed of the partition search (sbayes_amd.partsearch) at two shapes, 100 objects x K = 3 x 1 000 samples and 1 000 objects x
K = 5 x 10 000 samples, with 1 and 64 starts, against the NumPy checker on the same machine in the same run; prints one JSON
line and writes it to --out.

Samples are a planted partition with 25 % of the memberships scrambled per sample (tests/_partsearch_cases.noisy); the
starts are sbayes_amd.partsearch.make_starts' (the medoid by the checker's sums is replaced by sample 0: the tool times the
search, not the choice of its first start).  Device: the search kernel's time by HIP events (last_kernel_ms) and the call's
wall time (uploads of init and order, the launch, the copies back), the best of --repeats timed passes after a warming
one.  Host: tests/_partsearch_oracle.search, timed on the first --host-starts starts and SCALED to the number of starts (the
file says so).  Every output of those starts is compared for equality with the device's before anything is timed.
    python tools/partsearch_speed.py [--repeats 2] [--out profiles/partsearch/partsearch_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import partsearch                    # noqa: E402
from tests import _partsearch_cases as cases         # noqa: E402
from tests import _partsearch_oracle as orc          # noqa: E402

SHAPES = [("small", 100, 3, 1000), ("large", 1000, 5, 10000)]
STARTS = (1, 64)
MAX_SWEEPS = 32


def same(got, s, want):
    return bool(np.array_equal(got.labels[s], want.labels) and int(got.sweeps[s]) == want.sweeps and int(got.moves[s]) == want.moves
                and int(got.converged[s]) == want.converged and int(got.binder_sum[s]) == want.binder_sum and got.vi_sum[s] == want.vi_sum)


def one_shape(h, name, n, k, t, loss, repeats, host_starts):
    y, _ = cases.noisy(7000 + n, n, k, t)
    t0 = time.perf_counter()
    h.reset(k, n, t)
    h.append(orc.rows_of(y, k))
    upload_ms = (time.perf_counter() - t0) * 1e3
    init, order, _ = partsearch.make_starts(y, 0, k, max(STARTS), seed=5)
    m = min(host_starts, max(STARTS))
    t0 = time.perf_counter()
    want = [orc.search(y, k, loss, init[s], order[s], MAX_SWEEPS) for s in range(m)]
    host_s = (time.perf_counter() - t0) / m
    print(f"[{name} {loss}] host: {m} starts, {host_s:.2f} s each", file=sys.stderr, flush=True)
    rows = []
    for starts in STARTS:
        got = h.search(loss, init[:starts], order[:starts], MAX_SWEEPS)          # warms, sizes the buffers and is checked
        equal = all(same(got, s, want[s]) for s in range(min(m, starts)))
        call_ms = kernel_ms = float("inf")
        for _ in range(repeats):
            t0 = time.perf_counter()
            got = h.search(loss, init[:starts], order[:starts], MAX_SWEEPS)
            call_ms = min(call_ms, (time.perf_counter() - t0) * 1e3)
            kernel_ms = min(kernel_ms, got.kernel_ms)
        steps = int(got.sweeps.max()) * n                                          # object steps of the longest start
        row = {"shape": name, "objects": n, "clusters": k, "samples": t, "loss": loss, "starts": starts, "max_sweeps": MAX_SWEEPS,
               "sweeps_longest_start": int(got.sweeps.max()), "moves_total": int(got.moves.sum()), "all_converged": bool(got.converged.all()),
               "kernel_ms": round(kernel_ms, 3), "call_ms": round(call_ms, 3), "kernel_us_per_object_step_longest_start": round(kernel_ms * 1e3 / steps, 3),
               "upload_ms": round(upload_ms, 3), "host_numpy_ms_scaled": round(host_s * 1e3 * starts, 1), "host_starts_timed": m,
               "host_is_scaled": starts > m, "speedup_kernel": round(host_s * 1e3 * starts / kernel_ms, 1),
               "speedup_call": round(host_s * 1e3 * starts / call_ms, 1), "outputs_equal": equal, "starts_compared": min(m, starts),
               "mean_loss_best_start": float(got.loss_sum(loss).min()) / t, "mean_loss_first_start_init": None}
        ev = h.evaluate(init[:1], vi=False, binder=False)
        row["mean_loss_first_start_init"] = float((ev.vi_sum if loss == "vi" else ev.binder_sum)[0]) / t
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-starts", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=[name for name, *_ in SHAPES])
    ap.add_argument("--losses", nargs="+", default=list(cases.LOSSES))
    ap.add_argument("--out", default="profiles/partsearch/partsearch_speed.json")
    args = ap.parse_args()
    h = partsearch.SearchHandle()
    out = {"tool": "partsearch_speed", "host": "tests/_partsearch_oracle.search (NumPy), timed on host_starts_timed starts and scaled to `starts`",
           "timing": f"best of {args.repeats} timed passes after a warming one", "rows": []}
    try:
        for name, n, k, t in SHAPES:
            if name in args.shapes:
                for loss in args.losses:
                    out["rows"] += one_shape(h, name, n, k, t, loss, args.repeats, args.host_starts)
    finally:
        h.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
