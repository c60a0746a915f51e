"""The shared-operand epilogue of k_mixture_tuple_mfma (C = 2, 16 slots per block, FP4 operands; sbe_mixture_mfma.hip, SHARE).

It loads p1 and the two weight pairs of a slot once per column instead of once per table entry and must give the SAME BITS as
the per-entry epilogue (SBE_MFMA_SHARED=0), which runs in a fresh child process here.  The host picks the shared form only when
every slot of the launch has one component-1 group and at most two weight patterns (a per-slot flag kept with the tuple
tables); a launch with a slot that does not fit takes the per-entry epilogue.  Oracle: the NumPy restatement at 1e-10 relative."""
import importlib.util
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

pytestmark = pytest.mark.gpu

MARK = "shared operands"


def _bench():
    spec = importlib.util.spec_from_file_location("_bench_for_shared_epilogue", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _edge_engine(wl, batch):
    """bench.py's states, then edge cases in a few slots: every object in a cluster (no "no cluster" tuple: one weight pattern),
    and a zero probability on an observed state (log 0: the rare path, -inf)."""
    eng = _bench().setup_engine(wl, batch, 0)
    K = wl.clusters.shape[0]
    n_obj = wl.shape[0]
    rng = np.random.default_rng(77)
    all_objects = np.arange(n_obj, dtype=np.int32)
    for b in (3, 17, 40):
        eng.set_group_ids(b, 0, rng.integers(0, K, size=n_obj).astype(np.int32))
        eng.sample_source(b, b, all_objects, None, from_prior=True)
        eng.recount(b)
        for c in range(wl.n_components):
            eng.update_probs(b, c)
    p = eng.get_probs(5, 1)
    f = 0
    s = int(np.argmax(wl.features[:, f, :].sum(axis=0)))          # an observed state of feature 0
    p[0, f, s] = 0.0
    eng.set_probs(5, 1, p)
    return eng


def run_cases():
    """Results of the bit-identity cases under the current SBE_MFMA_SHARED; {name: (values, kernel name)}."""
    from sbayes_amd.synthetic import make_workload
    out = {}
    bench = _bench()
    wl = make_workload("headline")
    eng = bench.setup_engine(wl, 4096, 0)
    out["bench"] = (eng.mixture_loglik_batch(0, 4096), eng.last_mixture_kernel())
    out["b4090"] = (eng.mixture_loglik_batch(0, 4090), eng.last_mixture_kernel())
    eng.close()
    eng = _edge_engine(wl, 1024)
    out["edge"] = (eng.mixture_loglik_batch(0, 1024), eng.last_mixture_kernel())
    eng.close()
    wl1 = make_workload("cfg1")
    eng = bench.setup_engine(wl1, 4096, 0)
    out["cfg1"] = (eng.mixture_loglik_batch(0, 4096), eng.last_mixture_kernel())
    eng.close()
    return out


def _forced_old(module_file=__file__):
    """run_cases() of the test module `module_file` in a fresh child process with SBE_MFMA_SHARED=0 (also used by
    tests/test_gpu_mixture_log_range.py)."""
    with tempfile.TemporaryDirectory() as d:
        code = ("import importlib.util, sys, numpy as np\n"
                f"spec = importlib.util.spec_from_file_location('t', {str(Path(module_file))!r})\n"
                "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
                "out = m.run_cases()\n"
                "np.savez(sys.argv[1], **{k + '__v': v[0] for k, v in out.items()}, **{k + '__n': np.array(v[1]) for k, v in out.items()})\n")
        path = os.path.join(d, "old.npz")
        env = dict(os.environ, SBE_MFMA_SHARED="0")
        res = subprocess.run([sys.executable, "-c", code, path], env=env, cwd=str(REPO), capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        z = np.load(path)
        return {k[:-3]: (z[k], str(z[k[:-3] + "__n"])) for k in z.files if k.endswith("__v")}


@pytest.fixture(scope="module")
def both():
    return run_cases(), _forced_old()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case,tiles", [("bench", 3), ("b4090", 3), ("edge", 3), ("cfg1", 2)])
def test_shared_epilogue_gives_the_per_entry_bits(both, case, tiles):
    new, old = both
    (v1, n1), (v0, n0) = new[case], old[case]
    assert MARK in n1 and f"16 slots x M tiles {tiles}, C=2, {MARK}" in n1, n1
    assert MARK not in n0 and f"16 slots x M tiles {tiles}, C=2>" in n0, n0
    assert v1.shape == v0.shape
    assert _same_bits(v1, v0), np.flatnonzero(v1.view(np.uint64) != v0.view(np.uint64))[:10]
    if case == "edge":
        assert v1[5] == -np.inf                                         # the zero probability: log 0, as the reference
        assert np.all(np.isfinite(np.delete(v1, 5)))
    else:
        assert np.all(np.isfinite(v1))


def _oracle_check(eng, wl, values, slots):
    bench = _bench()
    bench.verify_results(eng, wl, slots, values[slots], "shared epilogue", tol=1e-10)


def test_bench_geometry_and_edges_against_the_oracle():
    from sbayes_amd.synthetic import make_workload
    wl = make_workload("headline")
    eng = _edge_engine(wl, 4096)
    got = eng.mixture_loglik_batch(0, 4096)
    assert f"16 slots x M tiles 3, C=2, {MARK}" in eng.last_mixture_kernel(), eng.last_mixture_kernel()
    slots = np.array([0, 1, 3, 15, 16, 17, 40, 511, 2048, 4079, 4080, 4095, 1234, 2345, 3456, 777])
    _oracle_check(eng, wl, got, slots)
    tail = eng.mixture_loglik_batch(0, 4090)                              # a last block of 10 slots
    assert _same_bits(tail, got[:4090])
    eng.close()


def test_cfg1_against_the_oracle():
    from sbayes_amd.synthetic import make_workload
    wl = make_workload("cfg1")
    eng = _bench().setup_engine(wl, 4096, 0)
    got = eng.mixture_loglik_batch(0, 4096)
    assert f"16 slots x M tiles 2, C=2, {MARK}" in eng.last_mixture_kernel(), eng.last_mixture_kernel()
    _oracle_check(eng, wl, got, np.array([0, 1, 2, 15, 16, 31, 100, 1000, 2047, 2048, 3000, 4000, 4080, 4093, 4094, 4095]))
    eng.close()


def test_two_confounder_groups_take_the_per_entry_epilogue():
    """C = 2 with a confounder of TWO groups: tuples differ in their component-1 group, so no slot fits the shared form (cfg1:
    K = 2, so 3 x 2 = 6 tuples still take 16 slots per block)."""
    from sbayes_amd.synthetic import make_workload
    wl = make_workload("cfg1")
    n_obj = wl.shape[0]
    two = np.zeros((2, n_obj), dtype=bool)
    two[0, : n_obj // 2] = True
    two[1, n_obj // 2:] = True
    conc = np.asarray(wl.concentration[1])
    wl.groups[1] = two
    wl.concentration[1] = np.concatenate([conc, conc], axis=0)[:2]
    eng = _bench().setup_engine(wl, 4096, 0)
    got = eng.mixture_loglik_batch(0, 4096)
    name = eng.last_mixture_kernel()
    assert "k_mixture_tuple_mfma" in name and "16 slots" in name and MARK not in name, name
    _oracle_check(eng, wl, got, np.array([0, 1, 2, 3, 15, 16, 17, 100, 255, 256, 511, 512, 700, 1000, 4094, 4095]))
    eng.close()


def test_changing_tables_keep_the_flag_right():
    """Objects move into and out of clusters through host updates and through the one-call step (sbe_step_delta), which
    rewrite the tuple tables in place; the next launches must still match the oracle (a stale flag would give NaN)."""
    from sbayes_amd.synthetic import make_workload
    wl = make_workload("headline")
    K = wl.clusters.shape[0]
    n_obj = wl.shape[0]
    B = 1024
    eng = _bench().setup_engine(wl, B + 3, 0)
    rng = np.random.default_rng(5)
    all_objects = np.arange(n_obj, dtype=np.int32)
    # host updates: a slot loses its "no cluster" objects, another gains many
    ids = rng.integers(0, K, size=n_obj).astype(np.int32)
    eng.set_group_ids(7, 0, ids)
    ids2 = ids.copy()
    ids2[: n_obj // 2] = -1
    eng.set_group_ids(9, 0, ids2)
    for b in (7, 9):
        eng.sample_source(b, b, all_objects, None, from_prior=True)
        eng.recount(b)
        for c in range(wl.n_components):
            eng.update_probs(b, c)
    got = eng.mixture_loglik_batch(0, B)
    assert MARK in eng.last_mixture_kernel(), eng.last_mixture_kernel()
    _oracle_check(eng, wl, got, np.array([0, 1, 7, 9, 15, 16, 100, 500, 511, 512, 700, 900, 1000, 1021, 1022, 1023]))
    # the one-call step: slot 7 (all in clusters) -> candidate B: a few objects leave their cluster; then candidate B + 1 from
    # slot 9: all of its "no cluster" objects join cluster 0 (the second pattern disappears)
    moved = np.array([3, 10, 11, 500], dtype=np.int32)
    eng.step_delta(7, B, moved_objects=moved, moved_cluster=np.full(moved.size, -1, dtype=np.int32))
    back = np.flatnonzero(ids2 < 0).astype(np.int32)
    eng.step_delta(9, B + 1, moved_objects=back, moved_cluster=np.zeros(back.size, dtype=np.int32))
    # slot 1 has both patterns and keeps them: a few objects leave clusters, a few join one (the O(moved) table update)
    ids1 = eng.get_group_ids(1, 0)
    out_ = np.flatnonzero(ids1 >= 0)[:3].astype(np.int32)
    in_ = np.flatnonzero(ids1 < 0)[:2].astype(np.int32)
    eng.step_delta(1, B + 2, moved_objects=np.concatenate([out_, in_]),
                   moved_cluster=np.array([-1, -1, -1, 1, 1], dtype=np.int32))
    for b, cur in ((B, 7), (B + 1, 9), (B + 2, 1)):
        eng.copy_slot(cur, b)
    got = eng.mixture_loglik_batch(0, B)
    assert MARK in eng.last_mixture_kernel(), eng.last_mixture_kernel()
    _oracle_check(eng, wl, got, np.array([0, 1, 7, 9, 15, 16, 100, 500, 511, 512, 700, 900, 1000, 1021, 1022, 1023]))
    eng.close()
