"""The EM cluster initializer on the device (include/sbe_em.h, sbayes_amd/em.py) against the fp64 restatement
(tests/_em_oracle.py) and the reference's recorded runs (tests/golden/em_init.npz).  Reads only tests/golden/."""
import ctypes as ct
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import _em_oracle as orc  # noqa: E402
from sbayes_amd import em  # noqa: E402
from sbayes_amd.engine import EngineError  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-300                 # relative on z, with a floor for entries near 0
GOLDEN = np.load(HERE / "golden" / "em_init.npz")


def golden(tag):
    g = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(tag + "/")}
    g["cost"] = g.get("cost")
    g["scale"] = float(g["scale"]) if "scale" in g else None
    return g


def synthetic(n, f, s, k, conf_groups=(), na=0.1, ragged=True, seed=0):
    """A random case: state index with NA, ragged applicable states, K clusters + confounder groups partitioning N."""
    rng = np.random.default_rng(seed)
    n_app = rng.integers(2, s + 1, size=f) if ragged else np.full(f, s)
    app = np.arange(s)[None, :] < n_app[:, None]
    x = (rng.random((n, f)) * n_app[None, :]).astype(np.uint8)
    x[rng.random((n, f)) < na] = s
    rows = [np.ones((k, n), dtype=bool)]
    for m in conf_groups:
        lab = rng.integers(0, m, size=n)
        rows.append(np.arange(m)[:, None] == lab[None, :])
    avail = np.concatenate(rows, axis=0)
    z0 = (rng.random(avail.shape) * avail)
    z0 = (z0 / z0.sum(axis=0)).astype(np.float32).astype(np.float64)
    return dict(x=x, applicable=app, groups_available=avail, n_clusters=k, z0=z0, cost=None, scale=None)


def with_geo(c, seed=1):
    rng = np.random.default_rng(seed)
    n = c["x"].shape[0]
    pts = rng.random((n, 2)) * 1000.0
    c = dict(c)
    c["cost"] = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    c["scale"] = 300.0
    return c


def handle(c):
    h = em.EmHandle(c["x"], np.asarray(c["applicable"], bool), np.asarray(c["groups_available"], bool), c["n_clusters"],
                    device=0)
    if c["cost"] is not None:
        h.set_geo_cost(c["cost"], c["scale"])
    return h


def check_against_restatement(c, n_steps=50, every=1):
    temps = orc.temperatures(50)[:n_steps]
    want = orc.em_steps(c["x"], c["applicable"], c["groups_available"], c["n_clusters"], c["z0"], temps, c["cost"], c["scale"])
    h = handle(c)
    try:
        z = np.array(c["z0"], dtype=np.float64)
        for i in range(0, n_steps, every):
            z = h.run(z, temps[i:i + every])
            np.testing.assert_allclose(z, want[min(i + every, n_steps) - 1], rtol=RTOL, atol=ATOL,
                                       err_msg=f"after step {min(i + every, n_steps) - 1}")
    finally:
        h.close()
    return z


def golden_case(tag):
    g = golden(tag)
    return dict(x=g["x"], applicable=g["applicable"], groups_available=g["groups_available"], n_clusters=int(g["n_clusters"]),
                z0=g["z0"].astype(np.float64), cost=g["cost"], scale=g["scale"])


@pytest.mark.parametrize("tag", ["cfg1", "south_america", "headline", "south_america_geo"])
def test_device_matches_restatement_at_every_step_on_golden_inputs(tag):
    check_against_restatement(golden_case(tag))


@pytest.mark.parametrize("name,case,steps", [
    ("stress_shaped_g51", lambda: synthetic(400, 60, 20, 10, conf_groups=(1, 20, 20), seed=3), 12),
    ("na_and_ragged", lambda: synthetic(37, 11, 7, 3, conf_groups=(1,), na=0.3, seed=4), 50),
    ("odd_tiles", lambda: synthetic(257, 65, 3, 2, conf_groups=(5,), seed=5), 50),
    ("g_is_k_plus_1", lambda: synthetic(129, 17, 4, 4, conf_groups=(1,), seed=6), 50),
    ("clusters_only", lambda: synthetic(70, 9, 5, 3, seed=7), 50),
    ("geo_prior", lambda: with_geo(synthetic(150, 20, 5, 3, conf_groups=(1, 4), seed=8)), 50),
    ("geo_k9_rows_over_8", lambda: with_geo(synthetic(90, 8, 4, 9, conf_groups=(1,), seed=9)), 20),
    ("states_254", lambda: synthetic(300, 3, 254, 2, conf_groups=(1,), na=0.05, ragged=False, seed=10), 10),
])
def test_device_matches_restatement_on_edge_shapes(name, case, steps):
    c = case()
    if name == "stress_shaped_g51":
        assert c["groups_available"].shape[0] == 51
    if name == "g_is_k_plus_1":
        assert c["groups_available"].shape[0] == c["n_clusters"] + 1
    check_against_restatement(c, n_steps=steps)


@pytest.mark.parametrize("tag,near_ties", [("cfg1", 0), ("south_america", 1), ("headline", 0), ("south_america_geo", 0)])
def test_device_against_the_reference_recording(tag, near_ties):
    """The rule of test_em_oracle_cpu.py: every snapshot within 2 r_i relative of the reference's float32 z, the final
    clusters equal except for objects within the near-tie bound."""
    from test_em_oracle_cpu import assert_z_close, step_bound, F32_TINY
    g = golden(tag)
    c = golden_case(tag)
    rec = {}
    orc.em_steps(c["x"], c["applicable"], c["groups_available"], c["n_clusters"], c["z0"], orc.temperatures(50), c["cost"],
                 c["scale"], record=rec)
    h = handle(c)
    try:
        z = c["z0"]
        temps = orc.temperatures(50)
        snaps = {}
        prev = 0
        for step in g["z_steps"]:
            z = h.run(z, temps[prev:step + 1])
            prev = step + 1
            snaps[int(step)] = z
    finally:
        h.close()
    floor = F32_TINY if g["z"].dtype == np.float32 else 0.0
    for j, step in enumerate(g["z_steps"]):
        assert_z_close(g["z"][j].astype(np.float64), snaps[int(step)], step_bound(g, rec, int(step)), floor, f"step {step}")
    k, m, t = int(g["n_clusters"]), int(g["min_size"]), int(g["total_size"])
    zr = snaps[49].astype(g["z"].dtype)
    r = step_bound(g, rec, 49)
    near = orc.decision_margin(zr, k, m, t) <= 2 * r / (1 - r)
    differ = (orc.discretize(zr, k, m, t) != g["clusters"]).any(axis=0)
    assert not (differ & ~near).any() and int(near.sum()) == near_ties


def test_bit_identical_across_runs_and_chunkings():
    for c in (golden_case("headline"), golden_case("south_america_geo")):
        temps = orc.temperatures(50)
        h = handle(c)
        try:
            a = h.run(c["z0"], temps)
            b = h.run(c["z0"], temps)
            z = c["z0"]
            for i in range(0, 50, 5):
                z = h.run(z, temps[i:i + 5])
            assert a.tobytes() == b.tobytes() == z.tobytes()
            assert h.last_kernel_ms() > 0
        finally:
            h.close()


def test_run_em_plain_function_and_zero_steps():
    c = synthetic(40, 6, 4, 2, conf_groups=(3,), seed=11)
    s = c["applicable"].shape[1]
    feats = np.zeros(c["x"].shape + (s,), dtype=bool)
    obs = c["x"] < s
    ii, jj = np.nonzero(obs)
    feats[ii, jj, c["x"][obs]] = True
    temps = orc.temperatures(50)
    z = em.run_em(feats, c["applicable"], c["groups_available"], 2, c["z0"], temps, device=0)
    want = orc.em_steps(c["x"], c["applicable"], c["groups_available"], 2, c["z0"], temps)[-1]
    np.testing.assert_allclose(z, want, rtol=RTOL, atol=ATOL)
    h = handle(c)
    try:
        assert h.run(c["z0"], temps[:0]).tobytes() == np.ascontiguousarray(c["z0"]).tobytes()
    finally:
        h.close()


def test_every_error_path_of_the_header():
    lib = em.load()
    c = synthetic(20, 4, 3, 2, conf_groups=(2,), seed=12)
    h = handle(c)
    try:
        temps = orc.temperatures(5)
        z0 = c["z0"].copy()
        out = np.empty_like(z0)
        # SBE_ERR_ARG: null pointers, step count, temperatures, scale, cost size
        assert lib.sbe_em_run(h._h, None, 5, temps.ctypes.data, out.ctypes.data) == 1
        assert lib.sbe_em_run(h._h, z0.ctypes.data, -1, temps.ctypes.data, out.ctypes.data) == 1
        assert lib.sbe_em_run(h._h, z0.ctypes.data, (1 << 20) + 1, temps.ctypes.data, out.ctypes.data) == 1
        assert lib.sbe_em_run(h._h, z0.ctypes.data, 5, None, out.ctypes.data) == 1
        bad_t = temps.copy()
        bad_t[3] = 0.0
        assert lib.sbe_em_run(h._h, z0.ctypes.data, 5, bad_t.ctypes.data, out.ctypes.data) == 1
        assert b"temperatures[3]" in lib.sbe_em_last_error(h._h)
        cost = np.zeros((20, 20))
        assert lib.sbe_em_set_geo_cost(h._h, cost.ctypes.data, -1.0) == 1
        ms = ct.c_float()
        assert lib.sbe_em_last_kernel_ms(h._h, None) == 1
        # SBE_ERR_DATA: z0 column summing to 0, a non-finite z0, a non-finite cost, a step with no finite group
        zbad = z0.copy()
        zbad[:, 7] = 0.0
        with pytest.raises(EngineError, match="column 7 of z_in sums to 0") as e:
            h.run(zbad, temps)
        assert e.value.code == 4
        zbad = z0.copy()
        zbad[1, 3] = np.nan
        with pytest.raises(EngineError, match="not finite"):
            h.run(zbad, temps)
        cost[2, 5] = np.inf
        assert lib.sbe_em_set_geo_cost(h._h, cost.ctypes.data, 10.0) == 4
        # the handle still works after refused calls
        z = h.run(z0, temps)
        assert np.all(np.isfinite(z)) and lib.sbe_em_last_kernel_ms(h._h, ct.byref(ms)) == 0
    finally:
        h.close()
    # a step with an object whose every available group has likelihood 0: state 2 of feature 0 is not applicable and
    # only object 4 has it, with z[0, 4] the smallest subnormal -- p underflows to 0, log p = -inf, the softmax is NaN
    c = synthetic(10, 2, 3, 1, seed=13, na=0.0, ragged=False)
    c["applicable"] = np.array([[True, True, False], [True, True, True]])
    c["x"][:, 0] = np.where(np.arange(10) == 4, 2, 0)
    z0 = c["z0"].copy()
    z0[0, 4] = 5e-324
    h = handle(c)
    try:
        with pytest.raises(EngineError, match="non-finite z") as e:
            h.run(z0, np.array([1.0]))
        assert e.value.code == 4
    finally:
        h.close()
    # SBE_ERR_ARG for a device index beyond the visible devices
    x, app, avail = c["x"], c["applicable"].view(np.uint8), c["groups_available"].view(np.uint8)
    hh = ct.c_void_p()
    assert lib.sbe_em_create(ct.byref(hh), 4096, 10, 2, 3, x.ctypes.data, app.ctypes.data, 1, 1, avail.ctypes.data) == 1
    assert b"out of range" in lib.sbe_em_last_error(None)


def test_handle_cache_per_data_object_and_fork_forgetting():
    from types import SimpleNamespace
    c = synthetic(30, 5, 4, 2, conf_groups=(3,), seed=14)
    s = c["applicable"].shape[1]
    feats = np.zeros(c["x"].shape + (s,), dtype=bool)
    obs = c["x"] < s
    ii, jj = np.nonzero(obs)
    feats[ii, jj, c["x"][obs]] = True
    conf = SimpleNamespace(group_assignment=c["groups_available"][2:])
    class Data:                               # (the reference's Data: a plain, weakly referenceable object)
        pass
    data = Data()
    data.features = SimpleNamespace(values=feats, na_values=~obs, states=c["applicable"])
    data.confounders = {"universal": conf}
    h1 = em.handle_for(data, 2)
    assert em.handle_for(data, 2) is h1
    h3 = em.handle_for(data, 3)
    assert h3 is not h1 and not h1._h
    em.release_all()
    assert not h3._h
