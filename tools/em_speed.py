"""Speed of the device EM initializer (sbayes_amd/em.py) per generate_clusters_em call (50 steps) against the fp64 NumPy
restatement (tests/_em_oracle.py) on the same host, for cfg1, south_america, headline and stress; writes
profiles/em/em_speed.json and prints it.

Device: wall time of EmHandle.run over 50 steps (z up, steps, z and the status word down) and the steps' device time by
HIP events (last_kernel_ms), best of --repeats after a warm-up call.  Host: the restatement's time per step, timed over
--oracle-steps steps (the stress shape is slow on the host).  The reference's own float32 time per step in the build
container is a static figure in DESIGN.md section 12.
    python tools/em_speed.py [--repeats 5] [--oracle-steps 3] [--only headline stress]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import _em_oracle as orc                          # noqa: E402
from sbayes_amd import em                        # noqa: E402
from sbayes_amd.synthetic import make_workload   # noqa: E402


def golden_case(tag):
    d = np.load(REPO / "tests" / "golden" / "em_init.npz")
    g = lambda k: d[f"{tag}/{k}"]                 # noqa: E731
    return g("x"), g("applicable"), g("groups_available"), int(g("n_clusters")), g("z0").astype(np.float64)


def workload_case(name):
    wl = make_workload(name)
    x = orc.state_index(wl.features, wl.na_values)
    k = wl.clusters.shape[0]
    avail = np.concatenate([np.ones((k, x.shape[0]), bool)] + [np.asarray(g, bool) for g in wl.groups[1:]], axis=0)
    rng = np.random.default_rng(0)
    z0 = rng.random(avail.shape) * avail
    return x, wl.states_per_feature.astype(bool), avail, k, (z0 / z0.sum(axis=0)).astype(np.float32).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle-steps", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out", default=str(REPO / "profiles" / "em" / "em_speed.json"))
    a = ap.parse_args()
    cases = {"cfg1": lambda: golden_case("cfg1"), "south_america": lambda: golden_case("south_america"),
             "headline": lambda: golden_case("headline"), "stress": lambda: workload_case("stress")}
    temps = em.temperatures(50)
    out = {"tool": "em_speed", "n_em_steps": 50, "repeats": a.repeats, "cases": []}
    for name, make in cases.items():
        if a.only and name not in a.only:
            continue
        x, app, avail, k, z0 = make()
        h = em.EmHandle(x, app, avail, k, device=0)
        try:
            h.run(z0, temps)                                          # warm-up (code objects, first-touch)
            walls, kms = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                h.run(z0, temps)
                walls.append(time.perf_counter() - t0)
                kms.append(h.last_kernel_ms())
        finally:
            h.close()
        steps = max(1, min(a.oracle_steps, 50))
        t0 = time.perf_counter()
        orc.em_steps(x, app, avail, k, z0, temps[:steps])
        host_step = (time.perf_counter() - t0) / steps
        n, f = x.shape
        row = dict(case=name, N=n, F=f, S=int(app.shape[1]), G=int(avail.shape[0]), K=k,
                   device_wall_ms_per_call=1e3 * min(walls), device_kernel_ms_per_call=min(kms),
                   device_kernel_us_per_step=1e3 * min(kms) / 50, restatement_ms_per_step=1e3 * host_step,
                   restatement_steps_timed=steps)
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
