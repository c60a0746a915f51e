"""Speed of the Gibbs weights step on the device (sbayes_amd.wgibbs: sbe_wgibbs_pair_counts + sbe_wgibbs_step) next to what
the parent path runs on the device for the same step (the reference's _propose around the device form of
source_lh_by_feature: two sbe_source_lh_by_feature calls with the new weights bound between them), timed in the same run
on the same engine; prints one JSON line and, with --out, writes it (profiles/wgibbs/wgibbs_speed.json).

Shapes: cfg1 (50 x 30, C = 2), south_america-sized (100 x 36, C = 3), headline (1000 x 200, C = 2) and stress
(5000 x 500, C = 4), states from sbayes_amd.synthetic (south_america-sized: a seeded state of that size).  Per shape, after
a warm-up, the median and the least of --repeats rounds of
  new      set_weights (the bind of the step's F * C floats), pair_counts, step
  parent   set_weights, source_lh_by_feature, set_weights (the proposal), source_lh_by_feature
each as the wall time of the synchronous calls (a host clock around calls that end in a wait for the device) and as the
device time of the same span (HIP events on the engine's stream, Engine.timer_start / timer_stop), and the wall time of
every single call.  The two sides alternate round by round.  The parent's host work around its two calls (the [N, F, C]
sum, the Dirichlet and beta log-pdfs) is not part of these figures: tools/wgibbs_host.py measures the host side.
The new calls' results are compared with tests/_wgibbs_oracle.py on the way (the timing doubles as a check).
    python tools/wgibbs_speed.py [--repeats 200] [--out profiles/wgibbs/wgibbs_speed.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from sbayes_amd import wgibbs                     # noqa: E402
from sbayes_amd.engine import Engine              # noqa: E402
from sbayes_amd.synthetic import make_workload    # noqa: E402
from tests import _wgibbs_oracle as worc          # noqa: E402

SHAPES = {"cfg1": "cfg1", "south_america_sized": (100, 36, 4, 3, (6,), False), "headline": "headline", "stress": "stress"}


def workload(spec):
    return make_workload(spec) if isinstance(spec, str) else make_workload("south_america_sized", shape=spec)


def spans(eng, calls, repeats):
    """calls: [(name, fn)].  -> per-call wall medians, and (median, least) of the whole round's wall and device time."""
    for _name, fn in calls:
        fn()
    per_call = {name: [] for name, _ in calls}
    walls, devs = [], []
    for _ in range(repeats):
        eng.timer_start()
        t_round = time.perf_counter()
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            per_call[name].append(time.perf_counter() - t0)
        walls.append(time.perf_counter() - t_round)
        devs.append(eng.timer_stop())
    return ({name: statistics.median(v) * 1e6 for name, v in per_call.items()},
            (statistics.median(walls) * 1e6, min(walls) * 1e6), (statistics.median(devs) * 1e3, min(devs) * 1e3))


def measure(name, spec, repeats):
    wl = workload(spec)
    n, f, _s = wl.shape
    c = wl.n_components
    rng = np.random.default_rng(7)
    i1, i2 = 0, 1
    t = 1.0
    alpha = np.ones((f, c))
    hc = np.stack([g.any(axis=0) for g in wl.groups], axis=1)
    patterns, pid, src = worc.state_of(hc, wl.source, wl.na_values)
    with Engine(wl.features, [g.shape[0] for g in wl.groups], n_slots=1, device=0) as eng:
        for comp in range(c):
            eng.set_groups(0, comp, wl.groups[comp])
        eng.set_source(0, wl.source)
        eng.set_weights(0, wl.weights)
        counts = wgibbs.pair_counts(eng, 0, i1, i2)
        assert np.array_equal(counts, worc.pair_counts(patterns, pid, src, wl.na_values, i1, i2))
        beta_ab = worc.beta_parameters(counts, np.ones((f, c), dtype=np.float32), i1, i2, t)
        a2 = rng.beta(beta_ab[:, 0], beta_ab[:, 1])
        u = rng.random(f, dtype=np.float32)
        w_out, accept, log_p = wgibbs.step(eng, 0, i1, i2, a2, u, alpha, beta_ab, t)
        want_out, want_accept, terms, w_new = worc.step(wl.weights, patterns, pid, src, wl.na_values, i1, i2, a2, u, alpha, beta_ab, t)
        clear = worc.log_margin(u, terms["log_p"]) > worc.device_band(terms, t)
        assert np.array_equal(accept[clear], want_accept[clear]) and w_out[clear].tobytes() == want_out[clear].tobytes()
        assert (np.abs(log_p - terms["log_p"]) <= worc.device_band(terms, t)).all()
        new_calls = [("set_weights", lambda: eng.set_weights(0, wl.weights)),
                     ("pair_counts", lambda: wgibbs.pair_counts(eng, 0, i1, i2)),
                     ("step", lambda: wgibbs.step(eng, 0, i1, i2, a2, u, alpha, beta_ab, t, want_log_p=False))]
        parent_calls = [("set_weights", lambda: eng.set_weights(0, wl.weights)),
                        ("source_lh_by_feature", lambda: eng.source_lh_by_feature(0)),
                        ("set_weights_proposal", lambda: eng.set_weights(0, w_new)),
                        ("source_lh_by_feature_proposal", lambda: eng.source_lh_by_feature(0))]
        rounds = {"new": [], "parent": []}
        for _ in range(4):                                  # the two sides alternate: drift of the host hits both
            rounds["new"].append(spans(eng, new_calls, repeats // 4))
            rounds["parent"].append(spans(eng, parent_calls, repeats // 4))
        out = dict(shape=name, n_objects=n, n_features=f, n_components=c, n_patterns=int(len(patterns)), repeats=repeats)
        for side, rs in rounds.items():
            out[side] = dict(
                call_us={k: round(statistics.median(r[0][k] for r in rs), 2) for k in rs[0][0]},
                round_wall_us=dict(median=round(statistics.median(r[1][0] for r in rs), 2), least=round(min(r[1][1] for r in rs), 2)),
                round_device_us=dict(median=round(statistics.median(r[2][0] for r in rs), 2), least=round(min(r[2][1] for r in rs), 2)))
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()
    result = dict(what="wall and device time of the Gibbs weights step's device calls (new) and of the parent path's device "
                       "calls for the same step (parent); microseconds; see tools/wgibbs_speed.py",
                  shapes=[measure(name, spec, args.repeats) for name, spec in SHAPES.items()])
    line = json.dumps(result)
    print(line)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
