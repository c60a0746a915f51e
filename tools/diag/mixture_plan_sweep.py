#!/usr/bin/env python3
"""Which form of the fused mixture kernel a launch runs, swept over shapes, launch sizes, options and experiment variables.

Uses the public Engine API only, so the same file runs on any commit: per (shape, environment) one fresh child process creates
an engine, loads two distinct states (every further slot is a copy of one of them: the selection does not look at values),
and launches once per (SBE_MIXTURE_* option, n).  Per process one JSON line {"job": ...} with what all its launches share (shape,
creation arguments [N, F, S, groups, slots], SBE_* environment, compute_units), then one JSON line per launch:
[option, n, P, KT, share_ok, name string or refusal, error code (0: launched), first 16 hex digits of the SHA-1 of the float64
results].  P, KT and share_ok are the facts of the launch, computed here in numpy from the arrays that were loaded (P = distinct
has_components rows, KT = distinct group tuples or 0 above 64, share_ok by the condition of tuples_share_operands).

    python tools/diag/mixture_plan_sweep.py --out sweep.json

tests/golden/mixture_plan_parent.json is this tool's output at the commit before plan_mixture (sbe_mixture_plan.h) existed;
tests/test_mixture_plan_cpu.py holds the planner to it.  The tool checks its own coverage: every form name, the two refusals
that a created engine can reach and both values of the shared-operand marker.  (The third refusal, "probability / weight tables
too large for LDS staging at tile width", cannot be reached through sbe_create: creation only keeps a tile width whose image
plus 8 KB fits 156 KB, and a launch adds at most 8 KB of staged ids to that image against a limit of 159 KB.)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(REPO))

N_LIST = (1, 2, 8, 15, 16, 31, 32, 64, 319, 320, 512, 513, 576, 1024)
N_FEW = (1, 2, 15, 16, 64, 1024)          # options whose choice moves with n only at the rows forms' thresholds (keeps the record small)
FULL_N = ("packed", "onehot", "packed_tuple_mfma")
OPTIONS = {"packed": 0, "onehot": 1, "packed_general": 2, "packed_tuple": 3, "onehot_general": 4, "packed_tuple_lds": 5,
           "packed_v2": 6, "packed_tuple_mfma": 7}
# make_workload(shape=(N, F, S, K, extra confounders, ragged states)); None: bench.load_workload(name)
SHAPES = {
    "cfg1": None, "south_america": None, "headline": None, "stress": None,
    "n500_c2": (500, 200, 10, 5, (), False), "n5000_c2": (5000, 200, 10, 5, (), False),
    "n500_c4": (500, 200, 10, 5, (20, 20), False), "n5000_c4": (5000, 200, 10, 5, (20, 20), False),
    "s130": (300, 40, 130, 3, (), False),                 # no prepared state stream: k_mixture_combo
    "f216": (1000, 216, 10, 5, (), False),                # last 64-feature tile holds 24 features (sub-row mode)
    "ragged": (400, 90, 8, 3, (), True),
    "direct": (300, 48, 40, 5, (60,), False),             # 67 groups x 40 states: not even a 16-feature tile fits LDS
    "wide": (200, 200, 10, 3, (3,), False),               # 9..16 group tuples, few objects per tuple
}
# (shape, environment, options): every option in the default environment, the experiment variables where they act
JOBS = [(name, {}, tuple(OPTIONS)) for name in SHAPES] + [(n, e, ("packed", "packed_general", "packed_tuple_mfma")) for n, e in [
    ("n5000_c4", {"SBE_ROWS_SORTED": "2"}), ("headline", {"SBE_MFMA_SMALL_SL4": "0"}), ("headline", {"SBE_MFMA_SPLIT": "3"}),
    ("wide", {"SBE_MFMA_WIDE_MIN_SHARE": "0"}),
]]
FORMS = ("k_mixture_tuple_mfma<", "k_mixture_tuple64<", "k_mixture_combo<", "k_mixture_rows<", ", pattern-sorted objects",
         "k_mixture_onehot_v2<", "k_mixture_v2<", ", direct tables", ", shared operands")
REFUSALS = ("matrix-pipe group-tuple kernel forced but not applicable", "group-tuple kernel forced but not applicable (")


def state_facts(groups):
    """(P, KT, share_ok) of one state from its per-component bool [G_c, N] group matrices."""
    ids = np.stack([np.where(g.any(axis=0), g.argmax(axis=0), -1) for g in groups], axis=1)          # [N, C]
    n_patterns = len(np.unique(ids >= 0, axis=0))
    tuples = np.unique(ids, axis=0)
    n_tuples = len(tuples) if len(tuples) <= 64 else 0
    share_ok = len(groups) == 2 and n_tuples > 0 and len(np.unique(tuples[:, 1])) == 1
    return n_patterns, n_tuples, bool(share_ok)


def child(shape_name, options, out_path):
    import bench
    from sbayes_amd.engine import Engine, EngineError
    from sbayes_amd.synthetic import make_state, make_workload
    spec = SHAPES[shape_name]
    wl = bench.load_workload(shape_name) if spec is None else make_workload(shape_name, shape=spec)
    n_obj, n_feat, n_states = wl.features.shape
    n_groups = [int(g.shape[0]) for g in wl.groups]
    slots = int(min(max(N_LIST), 4e9 // (n_obj * n_feat * n_states)))
    clusters, weights, source = make_state(wl.features, list(wl.groups[1:]), n_groups[0], 2)
    states = [(list(wl.groups), wl.weights, wl.source), ([clusters, *wl.groups[1:]], weights, source)]
    facts = [state_facts(groups) for groups, _w, _s in states]
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("SBE_")}
    with Engine(wl.features, n_groups, n_slots=slots, device=0) as eng, open(out_path, "w") as out:
        for c in range(len(n_groups)):
            eng.set_concentration(c, wl.concentration[c])
        for slot, (groups, w, src) in enumerate(states[:slots]):
            eng.load_state(slot, groups, w, source=src)
            for c in range(len(n_groups)):
                eng.update_probs(slot, c)
        for slot in range(2, slots):
            eng.copy_slot(slot, slot % 2)
        job = {"shape": shape_name, "create": [n_obj, n_feat, n_states, n_groups, slots], "env": env, "compute_units": int(eng.info()["compute_units"])}
        out.write(json.dumps({"job": job}) + "\n")
        for option in options:
            eng.set_option(kernel=OPTIONS[option])
            for n in (n for n in (N_LIST if option in FULL_N else N_FEW) if n <= slots or n == max(N_LIST)):
                n = min(n, slots)
                used = facts[:min(n, 2)]
                rec = [option, n, max(f[0] for f in used), 0 if any(f[1] == 0 for f in used) else max(f[1] for f in used), all(f[2] for f in used)]
                try:
                    res = np.asarray(eng.mixture_loglik_batch(0, n), dtype=np.float64)
                    rec += [eng.last_mixture_kernel(), 0, hashlib.sha1(res.tobytes()).hexdigest()[:16]]
                except EngineError as exc:
                    rec += [str(exc).split(": ", 1)[1], exc.code, ""]
                out.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", help="(internal) run one shape in this process")
    ap.add_argument("--options", default=",".join(OPTIONS), help="(internal) the child's options")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.options.split(","), args.out)
    lines = []
    for i, (shape_name, extra, options) in enumerate(JOBS):
        part = f"{args.out}.part{i}"
        env = {k: v for k, v in os.environ.items() if not k.startswith("SBE_")}
        env.update(extra)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--child", shape_name, "--options", ",".join(options), "--out", part]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            sys.exit(f"[sweep] {shape_name} {extra}: child exit code {rc}; stopping")
        lines += Path(part).read_text().splitlines()
        os.remove(part)
        print(f"[sweep] {shape_name} {extra}: {len(lines)} launches so far", flush=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    text = [rec[5] for rec in map(json.loads, lines) if isinstance(rec, list)]
    for want in FORMS + REFUSALS:
        assert any(want in t for t in text), f"no launch of the sweep shows {want!r}"
    assert any(t.startswith("k_mixture_tuple_mfma<") and ", shared operands" not in t for t in text), "no matrix-pipe launch without shared operands"
    print(f"[sweep] {len(text)} launches, every form and refusal seen -> {args.out}", flush=True)


if __name__ == "__main__":
    main()
