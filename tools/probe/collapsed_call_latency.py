"""Host time per call of the collapsed-likelihood and weight calls on the headline workload, next to calls whose kernels never
change (the completion floor, source_prior): one process, the calls interleaved over seven rounds of 1500, median per call in us,
one JSON line.  Run it once per process on each of two builds (SBAYES_AMD_LIB picks the library) and compare call minus floor:
the floor itself moves by up to 1.5 us from process to process (profiles/dcat/README.md)."""
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from sbayes_amd.engine import Engine                      # noqa: E402
from sbayes_amd.synthetic import make_workload           # noqa: E402

wl = make_workload("headline")
C = wl.n_components
with Engine(wl.features, [g.shape[0] for g in wl.groups], n_slots=2) as eng:
    for c in range(C):
        eng.set_concentration(c, wl.concentration[c])
    eng.load_state(0, wl.groups, wl.weights, source=wl.source)
    for c in range(C):
        eng.update_probs(0, c)
    eng.mixture_loglik(0)
    lib, h = eng._lib, eng._h
    calls = {
        "floor_empty_kernel": lambda: lib.sbe_test_roundtrip(h, 1, 0),
        "floor_mapped": lambda: lib.sbe_test_roundtrip(h, 1, 3),
        "source_prior": lambda: eng.source_prior(0),
        "collapsed_loglik_all": lambda: eng.collapsed_loglik_all(0),
        "collapsed_and_source_prior": lambda: eng.collapsed_and_source_prior(0),
        "set_weights": lambda: eng.set_weights(0, wl.weights),
        "one_call_step_weights": lambda: eng.step(0, 1, weights=wl.weights),
    }
    for fn in calls.values():
        for _ in range(300):
            fn()
    res = {k: [] for k in calls}
    for _rep in range(7):                                 # interleaved, so that drift hits the calls alike
        for k, fn in calls.items():
            n = 1500
            t = time.perf_counter()
            for _ in range(n):
                fn()
            res[k].append((time.perf_counter() - t) / n * 1e6)
    print(json.dumps({"lib": os.environ.get("SBAYES_AMD_LIB", ""), **{k: round(statistics.median(v), 2) for k, v in res.items()}}), flush=True)
