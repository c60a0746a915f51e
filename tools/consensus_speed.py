"""Speed of the posterior similarity, the scores and the comparison (sbayes_amd.consensus) at three shapes: a small one
(100 objects, K = 3, 1 000 samples), the headline's (1 000 objects, K = 5, 10 000 samples) and a large one (5 000
objects, K = 8, 10 000 samples), against the checker's NumPy forms on the same machine in the same run; prints one JSON
line and writes it to --out.

Samples are K planted blocks with 5 % of the bits flipped (tools/align_speed.samples).  Device: the kernels' time by HIP
events (last_kernel_ms) for the similarity, the scores of every sample and the comparison, and the wall time of the calls
(reset + append of all rows; similarity with the copy of the matrix; scores; compare).  Host: `Z.T @ Z` in float32 BLAS for
the counts (exact up to 2^24, as on the device; in two halves of the samples, added), the gather form of the scores (timed on --host-score-samples samples
and scaled), and the int64 NumPy form of the comparison.  Every device result is checked for equality against the host's.
    python tools/consensus_speed.py [--repeats 2] [--out profiles/consensus/consensus_speed.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from align_speed import samples                      # noqa: E402
from sbayes_amd import consensus                     # noqa: E402
from tests import _consensus_oracle as orc           # noqa: E402

SHAPES = [("small", 3, 100, 1000), ("headline", 5, 1000, 10000), ("large", 8, 5000, 10000)]


def host_counts(c):
    t0 = time.perf_counter()
    z = c.reshape(-1, c.shape[-1]).astype(np.float32)
    counts = (z.T @ z).astype(np.int32)
    return counts, time.perf_counter() - t0


def one_shape(h, name, k, n, s, repeats, host_score_samples):
    c = samples(k, n, s, 8000 + k * n)
    half = s // 2
    other, first_half_s = host_counts(c[:half])              # (the two halves: the second matrix of the comparison comes with them)
    rest, second_half_s = host_counts(c[half:])
    want, host_counts_s = other + rest, first_half_s + second_half_s
    print(f"[{name}] host counts {host_counts_s:.1f} s", file=sys.stderr, flush=True)
    m = min(host_score_samples, s)
    t0 = time.perf_counter()
    want_scores = orc.scores_gather(c[:m], want, s)
    host_scores_s = (time.perf_counter() - t0) * s / m
    t0 = time.perf_counter()
    want_cmp = orc.compare(want, s, other, half)
    host_compare_s = time.perf_counter() - t0
    print(f"[{name}] host scores and comparison done", file=sys.stderr, flush=True)
    best = {}
    for rep in range(repeats + 1):                         # (the first pass warms the runtime and sizes the buffers)
        t = {}
        t0 = time.perf_counter()
        h.reset(2, k, n, s)
        h.append(0, c)
        h.append(1, c[:half])
        t["upload_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        counts = h.similarity([0], slot=0)
        t["similarity_call_ms"] = (time.perf_counter() - t0) * 1e3
        t["similarity_kernel_ms"] = h.last_kernel_ms()
        t0 = time.perf_counter()
        scores = h.scores(0)
        t["scores_call_ms"] = (time.perf_counter() - t0) * 1e3
        t["scores_kernel_ms"] = h.last_kernel_ms()
        h.similarity([1], slot=1, copy=False)
        t0 = time.perf_counter()
        cmp = h.compare()
        t["compare_call_ms"] = (time.perf_counter() - t0) * 1e3
        t["compare_kernel_ms"] = h.last_kernel_ms()
        if rep == 0:
            first = dict(t)
            continue
        best = {key: min(v, best.get(key, v)) for key, v in t.items()}
    row = {"shape": name, "clusters": k, "objects": n, "samples": s, "elements": s * k,
           **{key: round(v, 3) for key, v in best.items()}, "first_pass_similarity_call_ms": round(first["similarity_call_ms"], 3),
           "host_counts_blas_f32_ms": round(host_counts_s * 1e3, 3), "host_scores_gather_ms_scaled": round(host_scores_s * 1e3, 3),
           "host_scores_samples_timed": m, "host_compare_ms": round(host_compare_s * 1e3, 3),
           "speedup_similarity_kernel": round(host_counts_s * 1e3 / best["similarity_kernel_ms"], 2),
           "speedup_similarity_call": round(host_counts_s * 1e3 / best["similarity_call_ms"], 2),
           "speedup_scores_kernel": round(host_scores_s * 1e3 / best["scores_kernel_ms"], 2),
           "speedup_scores_call": round(host_scores_s * 1e3 / best["scores_call_ms"], 2),
           "speedup_compare_call": round(host_compare_s * 1e3 / best["compare_call_ms"], 2),
           "counts_equal": bool(np.array_equal(counts, want)), "scores_equal": bool(np.array_equal(scores[:m], want_scores)),
           "compare_equal": bool(np.array_equal(cmp[0], want_cmp[0]) and np.array_equal(cmp[1], want_cmp[1]))}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-score-samples", type=int, default=200)
    ap.add_argument("--shapes", nargs="+", default=[name for name, *_ in SHAPES])
    ap.add_argument("--out", default="profiles/consensus/consensus_speed.json")
    args = ap.parse_args()
    h = consensus.ConsensusHandle()
    out = {"tool": "consensus_speed", "host_counts": "numpy float32 Z.T @ Z (BLAS)", "host_scores": "tests/_consensus_oracle.scores_gather",
           "shapes": []}
    try:
        for name, k, n, s in SHAPES:
            if name in args.shapes:
                out["shapes"].append(one_shape(h, name, k, n, s, args.repeats, args.host_score_samples))
    finally:
        h.close()
    line = json.dumps(out)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
