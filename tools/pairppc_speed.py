"""Speed of sbayes_amd.pairppc at the two shapes of tools/ppc_speed.py (1000 objects x 200 features x 10 states; the
south_america shape, 100 x 36 x 5), T = 1000 replicates each; prints one JSON line and writes it to --out.

Device: 2 warm-up and 5 timed repeats of add() on all replicates, with the kernel form left to the unit ("add") and forced to
each of the two forms ("add_sequential", "add_spread"): the pair kernel's time by HIP events (summed over the library
calls the block was split into) and the wall time of the synchronous call, smallest and median, with the number of library calls;
and the share of the call that is not the pair kernel (the host round trip of y_rep: upload, check and transpose).  The
yardsticks, measured in the same session: the screening's pair kernel (sbayes_amd.assoc) on one data set of the shape, smallest of
the same repeats, times T -- what a loop of sbe_assoc_compute calls would spend in its kernels alone; and the NumPy oracle
(tests/_pairppc_oracle.py) over --host-replicates replicates on the same host, scaled to T, with whether the device's counts of
those replicates follow the oracle's rule.  The replicates are the data with every column permuted on its own.
    python tools/pairppc_speed.py [--replicates 1000] [--out profiles/pairppc/pairppc_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import assoc, pairppc                # noqa: E402
from tests import _pairppc_oracle as orc             # noqa: E402

SHAPES = {"headline": dict(N=1000, F=200, S=10), "south_america": dict(N=100, F=36, S=5)}
WARMUP, REPEATS = 2, 5
SEED = 2501


def make_case(N, F, S, T, na_share=0.05):
    rng = np.random.default_rng(SEED)
    ns = rng.integers(2, S + 1, F).astype(np.int32)
    ns[0] = S
    latent = rng.integers(0, S, N)
    theta = rng.random(F) * 0.6
    x = np.empty((N, F), dtype=np.uint8)
    for k in range(F):
        x[:, k] = np.where(rng.random(N) < theta[k], latent % ns[k], rng.integers(0, ns[k], N))
    x[rng.random((N, F)) < na_share] = pairppc.NA
    y = np.repeat(x[None], T, axis=0)
    for t in range(T):
        y[t] = rng.permuted(x, axis=0)
    # (the permuted columns carry their NA cells along: each replicate has the data's number of NA per feature)
    return x, ns, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, default=3)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "pairppc" / "pairppc_speed.json")
    a = ap.parse_args()
    out = {"tool": "pairppc_speed", "replicates": a.replicates, "runs": []}
    h, ha = pairppc.PairHandle(0), assoc.AssocHandle(0)
    for name, shape in SHAPES.items():
        x, ns, y = make_case(T=a.replicates, **shape)
        t0 = time.perf_counter()
        h.set_data(x, ns)
        run = {"shape": name, **shape, "set_data_ms": round((time.perf_counter() - t0) * 1e3, 3), "observed_kernel_ms": round(h.last_kernel_ms(), 4),
               "replicates_per_library_call": h.max_replicates(), "library_calls": -(-a.replicates // h.max_replicates())}
        reads = {}
        for form in ("sequential", "spread", "auto"):                   # ("auto" last: the yardstick's ratio and the result below are its)
            h.set_form(form)
            walls, kernels = [], []
            for i in range(WARMUP + REPEATS):
                h.reset()
                t0 = time.perf_counter()
                h.add(y)
                if i >= WARMUP:
                    walls.append((time.perf_counter() - t0) * 1e3)
                    kernels.append(h.kernel_ms)
            s_pad, tile_pairs, launches = h.last_shape()
            run["add" if form == "auto" else "add_" + form] = {
                "kernel_ms": round(min(kernels), 4), "kernel_ms_median": round(float(np.median(kernels)), 4), "call_ms": round(min(walls), 4),
                "call_ms_median": round(float(np.median(walls)), 4), "warmup": WARMUP, "repeats": REPEATS, "s_pad": s_pad, "tile_pairs": tile_pairs,
                "launches_of_last_call": launches, "share_of_call_outside_the_pair_kernel": round(1.0 - min(kernels) / min(walls), 4)}
            res = h.result()
            reads[form] = b"".join(getattr(res, k).tobytes() for k in ("n_greater", "n_equal", "n_less", "n_degenerate", "sum", "sumsq"))
        run["forms_give_the_same_bytes"] = reads["sequential"] == reads["spread"] == reads["auto"]
        run["valid_pairs"], run["flagged_p_below_0.05"] = int(np.triu(res.valid_obs, 1).sum()), len(res.flagged(0.05))
        ms = []
        for i in range(WARMUP + REPEATS):
            ha.compute(x, ns)
            if i >= WARMUP:
                ms.append(ha.last_kernel_ms())
        run["assoc_yardstick"] = {"pair_kernel_ms_one_data_set": round(min(ms), 4), "times_replicates_ms": round(min(ms) * a.replicates, 3),
                                  "pairppc_kernel_over_yardstick": round(min(kernels) / (min(ms) * a.replicates), 4)}
        th = min(a.host_replicates, a.replicates)
        t0 = time.perf_counter()
        want = orc.check(x, ns, y[:th])
        seconds = time.perf_counter() - t0
        h.reset()
        h.add(y[:th])
        got, near = h.result(), orc.near(want)
        follows = all(bool((np.abs(getattr(got, k).astype(np.int64) - want[k]) <= near).all()) for k in ("n_greater", "n_equal", "n_less"))
        run["host"] = {"oracle_replicates": th, "oracle_s_per_replicate": round(seconds / (th + 1), 6),
                       "oracle_s_scaled_to_replicates": round(seconds / (th + 1) * a.replicates, 3), "device_counts_follow_the_oracle": follows}
        out["runs"].append(run)
    h.close()
    ha.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
