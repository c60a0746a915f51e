"""Speed of sbayes_amd.assoc.feature_association at the south_america (100 x 36), headline (1000 x 200 x 10) and stress
(5000 x 500 x 20) shapes against the pandas + SciPy loop of the reference's screening tool on the same host; prints one
JSON line and, with --out, writes it (profiles/assoc/assoc_speed.json).

Device: the synchronous call's wall time (check, transposition and upload of the codes, the launches, the five [F, F]
outputs copied back) and the pair kernel's time over all its launches by HIP events, each the median of --repeats calls
after a warm-up call.  Next to them the contraction's arithmetic floor: tile pairs x ceil(N / 64) MFMAs of 2 x 32 x 32 x
64 operations each at the FP4 peak (MI355X: 10 PFLOP/s dense), for the S_pad used -- what the matrix pipe alone would
take for the tiles computed.  Host: pd.crosstab + scipy.stats.chi2_contingency over a seeded sample of --host-pairs
pairs, scaled to the pair count (the full loop at the stress shape takes minutes).
    python tools/assoc_speed.py [--repeats 30] [--host-pairs 200] [--out profiles/assoc/assoc_speed.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from sbayes_amd import assoc                      # noqa: E402
from sbayes_amd.synthetic import make_workload    # noqa: E402

FP4_PEAK = 10.0e15                                # MI355X, FP4 MFMA, dense (operations per second)
MFMA_OPS = 2 * 32 * 32 * 64


def shapes():
    with np.load(REPO / "tests" / "golden" / "assoc.npz", allow_pickle=False) as z:
        yield "south_america", z["south_america_x"], z["south_america_n_states"]
    for name in ("headline", "stress"):
        features = make_workload(name).features
        yield name, assoc.state_codes(features), np.full(features.shape[1], features.shape[2], dtype=np.int32)


def host_loop(x, n_pairs, seed=0):
    """Seconds per pair of the tool's loop body over a seeded sample of pairs, and the sample's results."""
    import pandas as pd
    from scipy.stats import chi2_contingency
    f = x.shape[1]
    frame = pd.DataFrame({k: [None if c == assoc.NA else f"s{c:02d}" for c in x[:, k]] for k in range(f)}, dtype=object)
    iu = np.argwhere(np.triu(np.ones((f, f), dtype=bool), 1))
    sample = iu[np.random.default_rng(seed).choice(len(iu), size=min(n_pairs, len(iu)), replace=False)]
    out = []
    t0 = time.perf_counter()
    for i, j in sample:
        crosstab = pd.crosstab(frame[i], frame[j])
        if min(crosstab.shape) <= 1:
            out.append(None)
            continue
        out.append(chi2_contingency(crosstab))
    return (time.perf_counter() - t0) / len(sample), sample, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-pairs", type=int, default=200)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    h = assoc.handle_for(0)
    out = {"tool": "assoc_speed", "repeats": a.repeats, "host_pairs_sampled": a.host_pairs, "fp4_peak_ops_per_s": FP4_PEAK, "runs": []}
    for name, x, ns in shapes():
        n, f = x.shape
        res = assoc.feature_association(x, ns)                           # warm-up (code objects, buffers)
        walls, kernels = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            assoc.feature_association(x, ns)
            walls.append(time.perf_counter() - t0)
            kernels.append(h.last_kernel_ms() / 1e3)
        s_pad, tile_pairs, launches = h.last_shape()
        mfmas = tile_pairs * -(-n // 64)
        floor = mfmas * MFMA_OPS / FP4_PEAK
        per_pair, sample, ref = host_loop(x, a.host_pairs)
        for (i, j), r in zip(sample, ref):                                # the sample doubles as a check
            assert (r is not None) == bool(res.valid[i, j])
            if r is not None:
                assert abs(r.statistic - res.statistic[i, j]) <= 1e-12 * r.statistic and r.dof == res.dof[i, j]
        pairs = f * (f - 1) // 2
        wall, kern = statistics.median(walls), statistics.median(kernels)
        out["runs"].append({
            "shape": name, "n_objects": n, "n_features": f, "n_states_max": int(ns.max()), "pairs": pairs, "s_pad": s_pad,
            "tile_pairs": tile_pairs, "launches": launches, "mfma_instructions": mfmas,
            "call_wall_ms_median": wall * 1e3, "call_wall_ms_min": min(walls) * 1e3,
            "pair_kernel_ms_median": kern * 1e3, "pair_kernel_ms_min": min(kernels) * 1e3,
            "contraction_floor_ms_at_fp4_peak": floor * 1e3, "pair_kernel_over_floor": kern / floor,
            "host_pandas_scipy_ms_per_pair": per_pair * 1e3, "host_pairs_timed": len(sample),
            "host_pandas_scipy_s_scaled_to_all_pairs": per_pair * pairs,
            "speedup_call_over_host_loop": per_pair * pairs / wall,
        })
    line = json.dumps(out)
    print(line)
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
