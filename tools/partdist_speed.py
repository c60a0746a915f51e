"""Speed of the pairwise distances between cluster samples (sbayes_amd.partdist) at three shapes: a small one (100 objects,
K = 3, 1 000 samples), two runs (1 000 objects, K = 5, 2 x 1 000 samples) and the headline's (1 000 objects, K = 5, 10 000
samples), against NumPy on the same machine in the same run; prints one JSON line and writes it to --out.

Samples are K planted blocks with 5 % of the bits flipped (tools/align_speed.samples), every object kept only where exactly
one area holds it.  Device: the kernels' time by HIP events (last_kernel_ms) and the calls' wall time for the upload (reset
+ appends), for block() with its three outputs over all pairs (in row chunks of at most 2^25 entries, the copies to the
host included in the wall time), for block() with binder alone (the epilogue then stops before its float64 part) and for
sums().  Host: `Z @ Z.T` in float32 BLAS plus the checker's NumPy epilogue (tests/_partdist_oracle.measures), timed on the
first --host-rows samples against all and scaled to all rows.  Every
device result of those rows is compared for equality with the host's before anything is timed: binder, vi, sumsq, the
binder sums and the vi sums.  The contraction floor is tiles x N_pad / 64 MFMAs of 2 * 32 * 32 * 64 operations at 10 PFLOP/s.
    python tools/partdist_speed.py [--repeats 2] [--out profiles/partdist/partdist_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from align_speed import samples                      # noqa: E402
from sbayes_amd import partdist                      # noqa: E402
from tests import _partdist_oracle as orc            # noqa: E402
from tests._partdist_cases import exclusive          # noqa: E402

SHAPES = [("small", 3, 100, [1000]), ("two_runs", 5, 1000, [1000, 1000]), ("headline", 5, 1000, [10000])]
CHUNK_ENTRIES = 1 << 25
FP4_PEAK = 10e15                                     # operations per second of the FP4 matrix pipe


def host_rows(runs, m):
    """(binder, vi, sumsq) of the first m samples against all, and the seconds it took: float32 BLAS and the NumPy epilogue."""
    everything = np.concatenate(runs)
    t0 = time.perf_counter()
    k, n = everything.shape[1:]
    z = everything.reshape(-1, n).astype(np.float32)
    tables = (z[:m * k] @ z.T).astype(np.int64).reshape(m, k, len(everything), k).transpose(0, 2, 1, 3)
    sizes = everything.sum(axis=2, dtype=np.int64)
    pos = np.arange(len(everything))
    got = orc.measures(tables, sizes[:m], sizes, n, pos[:m, None] > pos[None, :])
    return got, time.perf_counter() - t0


def device_blocks(h, lengths, every=True):
    """block() over all pairs of all runs, with its three outputs or with binder alone: (wall ms, kernel ms)."""
    wall = kernel = 0.0
    for a, rows_a in enumerate(lengths):
        for b, rows_b in enumerate(lengths):
            step = max(1, CHUNK_ENTRIES // rows_b)
            for r0 in range(0, rows_a, step):
                t0 = time.perf_counter()
                h.block(a, r0, min(step, rows_a - r0), b, vi=every, sumsq=every)
                wall += (time.perf_counter() - t0) * 1e3
                kernel += h.last_kernel_ms()
    return wall, kernel


def one_shape(h, name, k, n, lengths, repeats, m):
    runs = [exclusive(samples(k, n, s, 9000 + k * n + r)) for r, s in enumerate(lengths)]
    total = sum(lengths)
    m = min(m, lengths[0])
    (want_b, want_v, want_s), host_s = host_rows(runs, m)
    print(f"[{name}] host: {m} rows against {total} in {host_s:.2f} s", file=sys.stderr, flush=True)
    at = np.cumsum([0] + lengths)
    best, equal = {}, {}
    for rep in range(repeats + 1):                         # (the first pass warms the runtime, sizes the buffers and checks)
        t = {}
        t0 = time.perf_counter()
        h.reset(len(runs), k, n, max(lengths))
        for r, run in enumerate(runs):
            h.append(r, run)
        t["upload_ms"] = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            for b in range(len(runs)):
                got = h.block(0, 0, m, b)
                cols = slice(at[b], at[b + 1])
                equal["binder_equal"] = equal.get("binder_equal", True) and bool(np.array_equal(got.binder, want_b[:, cols]))
                equal["vi_equal"] = equal.get("vi_equal", True) and bool(np.array_equal(got.vi, want_v[:, cols]))
                equal["sumsq_equal"] = equal.get("sumsq_equal", True) and bool(np.array_equal(got.sumsq, want_s[:, cols]))
        t["block_call_ms"], t["block_kernel_ms"] = device_blocks(h, lengths)
        t["binder_only_call_ms"], t["binder_only_kernel_ms"] = device_blocks(h, lengths, every=False)
        t0 = time.perf_counter()
        binder_sum, vi_sum = h.sums()
        t["sums_call_ms"] = (time.perf_counter() - t0) * 1e3
        t["sums_kernel_ms"] = h.last_kernel_ms()
        if rep == 0:
            want_bs = np.stack([want_b[:, at[b]:at[b + 1]].sum(axis=1) for b in range(len(runs))], axis=1)
            want_vs = np.stack([orc.tree_sum(want_v[:, at[b]:at[b + 1]]) for b in range(len(runs))], axis=1)
            equal["binder_sums_equal"] = bool(np.array_equal(binder_sum[:m], want_bs))
            equal["vi_sums_equal"] = bool(np.array_equal(vi_sum[:m], want_vs))
            first = dict(t)
            continue
        best = {key: min(v, best.get(key, v)) for key, v in t.items()}
    pad = partdist.padded_clusters(k)
    per_tile = 32 // pad
    tiles = sum(-(-a // per_tile) * -(-b // per_tile) for a in lengths for b in lengths)
    steps = -(-n // 256) * 4
    floor_ms = tiles * steps * 2 * 32 * 32 * 64 / FP4_PEAK * 1e3
    host_ms = host_s * 1e3 * total / m
    row = {"shape": name, "clusters": k, "objects": n, "samples": lengths, "pairs": total * total, "tiles": tiles, "steps_per_tile": steps,
           **{key: round(v, 3) for key, v in best.items()}, "first_pass_block_call_ms": round(first["block_call_ms"], 3),
           "contraction_floor_ms": round(floor_ms, 4), "block_kernel_over_floor": round(best["block_kernel_ms"] / floor_ms, 1),
           "host_blas_f32_and_numpy_ms_scaled": round(host_ms, 1), "host_rows_timed": m,
           "speedup_block_kernel": round(host_ms / best["block_kernel_ms"], 1), "speedup_block_call": round(host_ms / best["block_call_ms"], 1),
           "speedup_sums_call": round(host_ms / best["sums_call_ms"], 1), **equal}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=32)
    ap.add_argument("--shapes", nargs="+", default=[name for name, *_ in SHAPES])
    ap.add_argument("--out", default="profiles/partdist/partdist_speed.json")
    args = ap.parse_args()
    h = partdist.PartitionHandle()
    out = {"tool": "partdist_speed", "host": "numpy float32 Z @ Z.T (BLAS) + tests/_partdist_oracle.measures, a slice of rows scaled to all",
           "shapes": []}
    try:
        for name, k, n, lengths in SHAPES:
            if name in args.shapes:
                out["shapes"].append(one_shape(h, name, k, n, lengths, args.repeats, args.host_rows))
    finally:
        h.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
