"""Speed of the cost-based geo prior on the device (sbayes_amd.geo) against the host expression the reference runs
(SciPy's minimum_spanning_tree over the members' sub-matrix: tests/_geo_oracle.scipy_costs_per_object / scipy_geo_prior),
timed in the same run on the same machine; prints one JSON line and, with --out, writes it (profiles/geo/geo_speed.json).

Sizes (N objects, m members): (100, 20), (1000, 100), (1000, 300), (5000, 500), Euclidean costs of seeded points.  Per size:
one costs_per_object call and one geo_prior call on K = 5 masks -- the synchronous call's wall time (mask upload, the
launches, the result copied back) and the kernels' time by HIP events, each the median of --repeats calls after a warm-up
call -- next to the host expression's wall time on the same masks (median of --host-repeats).  Then geo_prior over 10 000
masks of the (1000, 100) shape in one call: masks per second over the wall time and over the kernels' time.  The results
of both sides are compared on the way (the timing doubles as a check).

--log-expit-out FILE measures the device's log_expit against scipy.special.log_expit over the fixed grid of
tests/_geo_oracle.log_expit_grid and writes the largest relative error (profiles/geo/log_expit_error.json: four times it is
the allowance tests/test_gpu_geo.py gives the device's exp / log1p).
    python tools/geo_speed.py [--repeats 30] [--host-repeats 10] [--out profiles/geo/geo_speed.json] [--log-expit-out FILE]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from sbayes_amd import geo                        # noqa: E402
from tests import _geo_oracle as orc              # noqa: E402

SIZES = [(100, 20), (1000, 100), (1000, 300), (5000, 500)]
K = 5
BATCH = 10000
KW = dict(aggregation="mean", probability_function="exponential")


def random_masks(rng, n, m, count):
    masks = np.zeros((count, n), dtype=bool)
    for row in masks:
        row[rng.choice(n, size=m, replace=False)] = True
    return masks


def timed(fn, repeats, kernel_ms=None):
    fn()                                            # warm-up (code objects, buffers)
    walls, kernels = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
        if kernel_ms is not None:
            kernels.append(kernel_ms())
    return out, statistics.median(walls) * 1e3, min(walls) * 1e3, (statistics.median(kernels) if kernels else None)


def log_expit_error(h, path):
    from scipy import special
    t = orc.log_expit_grid()
    got, want = h.log_expit(t), special.log_expit(t)
    rel = np.abs(got - want) / np.abs(want)
    worst = int(np.argmax(rel))
    out = {"tool": "geo_speed --log-expit-out", "against": "scipy.special.log_expit", "grid_points": int(t.size),
           "grid": "tests/_geo_oracle.log_expit_grid", "largest_relative_error": float(rel[worst]), "at_t": float(t[worst]),
           "in_units_of_2^-53": float(rel[worst] / orc.U), "share_of_arguments_bit_equal": float(np.mean(got == want))}
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=10)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--log-expit-out", type=Path, default=None)
    a = ap.parse_args()
    h = geo.handle_for(0)
    out = {"tool": "geo_speed", "repeats": a.repeats, "host_repeats": a.host_repeats, "k_masks": K, "runs": []}
    if a.log_expit_out is not None:
        out["log_expit"] = log_expit_error(h, a.log_expit_out)
    costs = {}
    for n, m in SIZES:
        rng = np.random.default_rng(1000 * n + m)
        if n not in costs:
            costs[n] = orc.euclidean_cost(np.random.default_rng(n).uniform(0, 1000, size=(n, 2)))
        cost = costs[n]
        t0 = time.perf_counter()
        h.set_cost(cost)
        upload_ms = (time.perf_counter() - t0) * 1e3
        masks = random_masks(rng, n, m, K)
        scale = float(cost.mean())
        dev_po, po_wall, po_min, po_kernel = timed(lambda: h.costs_per_object(masks[0], scale, **KW), a.repeats, h.last_kernel_ms)
        host_po, hpo_wall, hpo_min, _ = timed(lambda: orc.scipy_costs_per_object(cost, masks[0], scale, **KW), a.host_repeats)
        dev_gp, gp_wall, gp_min, gp_kernel = timed(lambda: h.prior(masks, scale, **KW), a.repeats, h.last_kernel_ms)
        host_gp, hgp_wall, hgp_min, _ = timed(lambda: orc.scipy_geo_prior(cost, masks, scale, **KW), a.host_repeats)
        assert np.allclose(dev_po, host_po, rtol=1e-12, atol=1e-12) and np.allclose(dev_gp, host_gp, rtol=1e-12, atol=1e-12)
        out["runs"].append({
            "n_objects": n, "members": m, "lds_path": m <= geo.LDS_MEMBERS, "set_cost_ms": upload_ms,
            "costs_per_object": {"device_call_wall_ms_median": po_wall, "device_call_wall_ms_min": po_min, "device_kernels_ms_median": po_kernel,
                                 "host_scipy_ms_median": hpo_wall, "host_scipy_ms_min": hpo_min, "speedup_call_over_host": hpo_wall / po_wall},
            "geo_prior_k5": {"device_call_wall_ms_median": gp_wall, "device_call_wall_ms_min": gp_min, "device_kernels_ms_median": gp_kernel,
                             "host_scipy_ms_median": hgp_wall, "host_scipy_ms_min": hgp_min, "speedup_call_over_host": hgp_wall / gp_wall},
        })
    n, m = 1000, 100
    h.set_cost(costs[n])
    masks = random_masks(np.random.default_rng(77), n, m, BATCH)
    scale = float(costs[n].mean())
    dev, wall, wall_min, kernel = timed(lambda: h.prior(masks, scale, **KW), max(3, a.repeats // 5), h.last_kernel_ms)
    t0 = time.perf_counter()
    host = orc.scipy_geo_prior(costs[n], masks[:200], scale, **KW)
    host_ms_per_mask = (time.perf_counter() - t0) * 1e3 / 200
    assert np.allclose(dev[:200], host, rtol=1e-12, atol=1e-12)
    launches, lds_masks = h.last_shape()
    out["batched"] = {"n_objects": n, "members": m, "masks": BATCH, "launches": launches, "lds_masks": lds_masks,
                      "device_call_wall_ms_median": wall, "device_call_wall_ms_min": wall_min, "last_kernel_ms_median": kernel,
                      "masks_per_second_call": BATCH / (wall / 1e3), "masks_per_second_kernel": BATCH / (kernel / 1e3),
                      "host_scipy_ms_per_mask_over_200": host_ms_per_mask, "host_masks_per_second": 1e3 / host_ms_per_mask}
    line = json.dumps(out)
    print(line)
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
