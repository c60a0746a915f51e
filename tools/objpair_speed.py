"""Speed of sbayes_amd.objpair at the two shapes of tools/ppc_speed.py (1000 objects x 200 features x 10 states; the
south_america shape, 100 x 36 x 5), T = 1000 replicates each; prints one JSON line and writes it to --out.

The replicates are those of the posterior predictive check of a seeded case (sbayes_amd.ppc).  Device: 2 warm-up and 5 timed
repeats of add() on all replicates: the replicate kernel (contraction and tally, one kernel) by HIP events, summed over the
library calls the block was split into, and the wall time of the synchronous call, smallest and median; what the call takes
beside that kernel is the upload, the pack kernel and the waits ("call_minus_kernel_ms": the handle's events do not separate
them).  The contraction alone is bounded from the shapes: "mfma_floor_ms" is the FP4 multiply-adds of the call's tile pairs over
the matrix pipe's peak, so kernel_ms over it says how far the kernel is from being bound by the contraction.  result() (the
mirror kernels and the copy back of the seven [N, N] arrays) is timed the same way, and add(agree_rep=True) once.  In the same
session, on the same replicates: pairppc's add (its pair kernel) and spatial's add with 8 quantile classes over all pairs.
Host, on the same machine, each over --host-replicates replicates and that figure SCALED to T (neither is run on all of them):
the NumPy checker (tests/_objpair_oracle.py), and a float32 BLAS product Y Y^T of the one-hot rows, with whether the device's
counts of those replicates equal both.
    python tools/objpair_speed.py [--replicates 1000] [--out profiles/objpair/objpair_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from sbayes_amd import objpair, pairppc, ppc, spatial   # noqa: E402
from tests import _objpair_oracle as orc                # noqa: E402
from tests import _predict_oracle as predict_orc        # noqa: E402

SHAPES = {"headline": dict(N=1000, F=200, S=10, C=2, K=5, group_counts=[10]),
          "south_america": dict(N=100, F=36, S=5, C=3, K=3, group_counts=[1, 6])}
WARMUP, REPEATS = 2, 5
SEED = 3101
PEAK_FP4_FLOPS = 10e15                                   # dense FP4 on the matrix pipe of an MI355X (the vendor's figure)


def timed(call, reset, kernel_ms):
    """(walls, kernels) of REPEATS calls after WARMUP, in milliseconds; kernel_ms(): the unit's device time of the last call."""
    walls, kernels = [], []
    for i in range(WARMUP + REPEATS):
        reset()
        t0 = time.perf_counter()
        call()
        if i >= WARMUP:
            walls.append((time.perf_counter() - t0) * 1e3)
            kernels.append(kernel_ms())
    return walls, kernels


def summary(walls, kernels, calls):
    return {"kernel_ms": round(min(kernels), 4), "kernel_ms_median": round(float(np.median(kernels)), 4), "call_ms": round(min(walls), 4),
            "call_ms_median": round(float(np.median(walls)), 4), "call_minus_kernel_ms": round(min(walls) - min(kernels), 4), "library_calls": calls,
            "warmup": WARMUP, "repeats": REPEATS}


def one_hot(y, n_states):
    """float32 [N, E] one-hot rows of one data set (NA: no element)."""
    off = np.concatenate([[0], np.cumsum(n_states)[:-1]])
    rows = np.zeros((y.shape[0], int(np.sum(n_states))), dtype=np.float32)
    i, f = np.nonzero(y != orc.NA)
    rows[i, off[f] + y[i, f]] = 1.0
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--host-replicates", type=int, default=3)
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent.parent / "profiles" / "objpair" / "objpair_speed.json")
    a = ap.parse_args()
    out = {"tool": "objpair_speed", "replicates": a.replicates, "seed": SEED, "peak_fp4_flops": PEAK_FP4_FLOPS, "runs": []}
    hp, h, hq, hs = ppc.PpcHandle(0), objpair.ObjPairHandle(0), pairppc.PairHandle(0), spatial.SpatialHandle(0)
    for name, shape in SHAPES.items():
        case = predict_orc.random_case(1, T=a.replicates, out_share=0.2, na_share=0.05, **shape)
        hp.set_data(case["codes"], case["groups"], case["n_groups"], shape["S"], shape["K"])
        hp.check(case["clusters"], case["weights"], case["tables"], seed=SEED, replicates=True)
        y = hp.result().y_rep
        n, f, t_n = shape["N"], shape["F"], a.replicates
        n_states = np.full(f, shape["S"], dtype=np.int32)
        t0 = time.perf_counter()
        h.set_data(case["codes"], n_states)
        run = {"shape": name, **{k: v for k, v in shape.items() if k in "NFS"}, "E": int(n_states.sum()),
               "set_data_ms": round((time.perf_counter() - t0) * 1e3, 3), "observed_kernel_ms": round(h.last_kernel_ms(), 4),
               "replicates_per_library_call": h.max_replicates(), "replicate_bytes": objpair.replicate_bytes(n, f, int(n_states.sum()))}
        walls, kernels = timed(lambda: h.add(y), h.reset, lambda: h.kernel_ms)
        e_pad, tile_pairs, launches = h.last_shape()
        run["add"] = summary(walls, kernels, -(-t_n // h.max_replicates()))
        run["last_shape"] = {"e_pad": e_pad, "tile_pairs": tile_pairs, "launches_of_last_call": launches}
        flops = 2.0 * tile_pairs * 32 * 32 * e_pad * t_n
        run["mfma_floor_ms"] = round(flops / PEAK_FP4_FLOPS * 1e3, 4)
        run["kernel_over_mfma_floor"] = round(run["add"]["kernel_ms"] / (flops / PEAK_FP4_FLOPS * 1e3), 2)
        run["pairs_times_replicates_per_kernel_s"] = round(n * (n - 1) / 2 * t_n / (run["add"]["kernel_ms"] * 1e-3), 0)
        walls, _k = timed(h.result, lambda: None, lambda: 0.0)
        run["result_ms"] = {"call_ms": round(min(walls), 4), "call_ms_median": round(float(np.median(walls)), 4), "bytes": 36 * n * n}
        t0 = time.perf_counter()
        h.reset()
        h.add(y[:min(t_n, 50)], agree_rep=True)
        run["add_with_agree_rep_50"] = {"call_ms": round((time.perf_counter() - t0) * 1e3, 3), "kernel_ms": round(h.kernel_ms, 4), "replicates": min(t_n, 50)}
        res = (h.reset(), h.add(y), h.result())[2]
        run["flagged_at_0.05"] = len(res.flagged(0.05))
        # the siblings on the same replicates, in the same session
        hq.set_data(case["codes"], n_states)
        walls, kernels = timed(lambda: hq.add(y), hq.reset, lambda: hq.kernel_ms)
        run["pairppc_add"] = summary(walls, kernels, -(-t_n // hq.max_replicates()))
        band, b = spatial.bands_from_costs(spatial.plane_distances(np.random.default_rng(SEED).random((n, 2))), n_bands=8)
        hs.set_data(case["codes"], n_states, band, b)
        walls, kernels = timed(lambda: hs.add(y), hs.reset, lambda: hs.kernel_ms)
        run["spatial_bands8_add"] = summary(walls, kernels, -(-t_n // hs.call_replicates()))
        # the host, on a few replicates and scaled
        th = min(a.host_replicates, t_n)
        t0 = time.perf_counter()
        want = [orc.statistics(y[t])[0] for t in range(th)]
        oracle_s = (time.perf_counter() - t0) / th
        t0 = time.perf_counter()
        blas = []
        for t in range(th):
            rows = one_hot(y[t], n_states)
            c = rows @ rows.T
            np.fill_diagonal(c, 0)
            blas.append(c)
        blas_s = (time.perf_counter() - t0) / th
        h.reset()
        got = h.add(y[:th], agree_rep=True)
        run["host"] = {"replicates": th, "scaled": True, "oracle_s_per_replicate": round(oracle_s, 6), "oracle_s_scaled_to_replicates": round(oracle_s * t_n, 3),
                       "blas_f32_s_per_replicate": round(blas_s, 6), "blas_f32_s_scaled_to_replicates": round(blas_s * t_n, 3),
                       "device_equals_oracle": bool(all(np.array_equal(got[t], want[t]) for t in range(th))),
                       "device_equals_blas": bool(all(np.array_equal(got[t], blas[t].astype(np.int32)) for t in range(th))),
                       "device_call_faster_than_scaled_blas": bool(run["add"]["call_ms"] < blas_s * t_n * 1e3)}
        out["runs"].append(run)
    for handle in (hs, hq, h, hp):
        handle.close()
    line = json.dumps(out)
    print(line, flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
