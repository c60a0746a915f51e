"""Speed of the within-run label alignment (sbayes_amd.align) at S = 10 000 samples per run for 1, 8 and 64 runs, at the
south_america size (K = 3, N = 100), the headline size (K = 5, N = 1000) and K = 8 at sbe_align_max_objects(8), against
the host restatement on the same machine in the same run; prints one JSON line and writes it to --out.

Samples are K planted blocks with 5 % of the bits flipped and the rows of every sample shuffled; every run of a shape
holds the same samples (the kernel's time does not depend on which run a sample is in).  Device: the within-run kernel's
time by HIP events (last_kernel_ms), per step (/ S), and the wall time of the whole call (reset, the appends of every
run, within).  Host: one run, NumPy matmul + SciPy's linear_sum_assignment per step as the reference does it (the
checker's solver where SciPy is not installed), times the number of runs.
    python tools/align_speed.py [--samples 10000] [--runs 1 8 64] [--out profiles/align/align_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import align                     # noqa: E402
from tests import _align_cases as cases          # noqa: E402
from tests import _align_oracle as orc           # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment
    HOST = "numpy matmul + scipy linear_sum_assignment"
except ImportError:                              # (the checker's brute force: slower, the same permutations off ties)
    linear_sum_assignment = None
    HOST = "numpy matmul + tests/_align_oracle.best_permutation"


def samples(k, n, s, seed):
    rng = np.random.default_rng(seed)
    base = np.zeros((k, n), dtype=np.uint8)
    at = 0
    for i, size in enumerate(cases.block_sizes(k, n)):
        base[i, at:at + size] = 1
        at += size
    out = np.empty((s, k, n), dtype=np.uint8)
    for s0 in range(0, s, 256):
        m = min(256, s - s0)
        c = base[None] ^ (rng.random((m, k, n)) < 0.05).astype(np.uint8)
        order = np.argsort(rng.random((m, k)), axis=1)
        out[s0:s0 + m] = np.take_along_axis(c, order[:, :, None], axis=1)
    return out


def host_within(c, seed_rows):
    """The contract with the reference's solver; returns (perms, seconds)."""
    t0 = time.perf_counter()
    x = c.astype(np.int64)
    m = min(seed_rows, len(x))
    w = max(m, 1)
    total = x[:m].sum(axis=0)
    perms = np.empty(x.shape[:2], dtype=np.int64)
    for s in range(len(x)):
        d = total @ x[s].T
        p = linear_sum_assignment(d, maximize=True)[1] if linear_sum_assignment else orc.best_permutation(d)
        total += w * x[s][p]
        perms[s] = p
    return perms, time.perf_counter() - t0


def one_shape(h, k, n, s, run_counts, seed_rows, repeats):
    c = samples(k, n, s, 7000 + k * n)
    want, host_s = host_within(c, seed_rows)
    rows = []
    for r in run_counts:
        walls, kernels, perms = [], [], None
        for _ in range(repeats + 1):                 # (the first pass warms the runtime and sizes the buffers)
            t0 = time.perf_counter()
            h.reset(r, k, n, s)
            for run in range(r):
                h.append(run, c)
            perms = h.within(seed_rows)
            walls.append(time.perf_counter() - t0)
            kernels.append(h.last_kernel_ms())
        kern, wall = min(kernels[1:]), min(walls[1:])
        rows.append({"clusters": k, "objects": n, "samples": s, "runs": r, "seed_rows": seed_rows,
                     "kernel_ms": round(kern, 3), "kernel_us_per_step": round(kern * 1e3 / s, 3),
                     "kernel_us_per_step_per_run": round(kern * 1e3 / s / r, 3),
                     "upload_and_within_ms": round(wall * 1e3, 3), "first_call_ms": round(walls[0] * 1e3, 3),
                     "host_s_one_run": round(host_s, 3), "host_us_per_step": round(host_s * 1e6 / s, 3),
                     "host_s_all_runs_scaled": round(host_s * r, 3),
                     "speedup_kernel": round(host_s * r / (kern / 1e3), 2), "speedup_upload_and_within": round(host_s * r / wall, 2),
                     "steps_equal_to_host": int(np.count_nonzero((perms[0] == want).all(axis=1))),
                     "runs_equal_to_run_0": int(sum(np.array_equal(p, perms[0]) for p in perms))})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--runs", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--seed-rows", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default="profiles/align/align_speed.json")
    args = ap.parse_args()
    shapes = [("south_america", 3, 100), ("headline", 5, 1000), ("k8_max_objects", 8, align.max_objects(8))]
    h = align.AlignHandle()
    out = {"tool": "align_speed", "host": HOST, "max_objects_k8": align.max_objects(8), "shapes": []}
    try:
        for name, k, n in shapes:
            for row in one_shape(h, k, n, args.samples, args.runs, args.seed_rows, args.repeats):
                out["shapes"].append({"shape": name, **row})
    finally:
        h.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
