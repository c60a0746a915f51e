"""The mixture kernels' fp64 logs ENTRY BY ENTRY over the float32 range (values, layouts, reference and the derived bounds:
tests/_mixlog_cases.py; the same model without a device: tests/test_mixlog_model_cpu.py).

A state of layout A has one table entry with a count, so a launch returns N log q_b for a chosen float32 q_b per slot: one
row of the matrix-pipe kernel's 1024-row log table, one series, one exponent -- where every other mixture test sees a sum of
thousands of logs at 1e-10.  Layout B puts two entries through the shared-operand epilogue, layout C one per group tuple
through the wide forms with exponents 2^-149 .. 2^0 side by side in a lane; the vector-pipe forms run the same values in
both log modes, and one geometry close under the matrix-pipe form's 32-bit exponent-sum guard runs with the largest and the
smallest exponents.  Every generated value is compared (the counts are asserted); nothing is skipped or filtered.

Each test prints `[mixlog]` lines: the largest error over bound per exponent class and per first / last / other table row,
with the value where it occurs."""
import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from sbayes_amd.engine import (LOG_PER_OBS, LOG_PRODUCT, MIXTURE_ONEHOT, MIXTURE_ONEHOT_GENERAL, MIXTURE_PACKED, MIXTURE_PACKED_GENERAL,
                               MIXTURE_PACKED_TUPLE, MIXTURE_PACKED_TUPLE_LDS, MIXTURE_PACKED_TUPLE_MFMA, MIXTURE_PACKED_V2, Engine, EngineError)
from tests import _mixlog_cases as mc

pytestmark = pytest.mark.gpu

SLOTS = 4096                                     # slots per engine; the values go through in chunks of this many
MFMA = "k_mixture_tuple_mfma"
VECTOR_FORMS = {"MIXTURE_PACKED": MIXTURE_PACKED, "MIXTURE_ONEHOT": MIXTURE_ONEHOT, "MIXTURE_PACKED_GENERAL": MIXTURE_PACKED_GENERAL,
                "MIXTURE_ONEHOT_GENERAL": MIXTURE_ONEHOT_GENERAL, "MIXTURE_PACKED_V2": MIXTURE_PACKED_V2,
                "MIXTURE_PACKED_TUPLE": MIXTURE_PACKED_TUPLE, "MIXTURE_PACKED_TUPLE_LDS": MIXTURE_PACKED_TUPLE_LDS}
VECTOR_BATCH = 256                               # below the 320 states from which MIXTURE_PACKED itself takes the matrix pipe


# ---- engines and launches -----------------------------------------------------------------------------------------------
def _engine_a(N, n_slots):
    """Layout A with n_slots identical states; the tests re-set only the probabilities per slot."""
    feats, n_groups, groups = mc.layout_a(N)
    eng = Engine(feats, n_groups, n_slots=n_slots)
    eng.load_state(0, groups, np.ones((1, 1), dtype=np.float32), probs=[mc.probs_a(0.5, False)])
    for b in range(1, n_slots):
        eng.copy_slot(b, 0)
    return eng


def _set_a(eng, q, first):
    """Slot b <- q[b]; the unobserved state gets 1 - q in the odd cases and exactly 0 in the even ones (`first`: index of q[0]
    among all values).  It has no observations: it contributes nothing either way."""
    p = np.stack([mc.probs_a(x, ((first + b) & 1) == 0) for b, x in enumerate(q)])
    for b in range(q.size):
        eng.set_probs(b, 0, p[b])


def _mfma_launch(eng, n, expect=""):
    got = eng.mixture_loglik_batch(0, n)
    name = eng.last_mixture_kernel()
    assert MFMA in name and expect in name, name
    return got


def _run_a_mfma(N, q):
    """Every value of q through the matrix-pipe form at N objects -> (results, results of a second launch)."""
    out, again = np.empty(q.size), np.empty(q.size)
    with _engine_a(N, min(SLOTS, q.size)) as eng:
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        for lo in range(0, q.size, SLOTS):
            chunk = q[lo:lo + SLOTS]
            _set_a(eng, chunk, lo)
            out[lo:lo + chunk.size] = _mfma_launch(eng, chunk.size)
            again[lo:lo + chunk.size] = _mfma_launch(eng, chunk.size)
    return out, again


def _engine_b():
    """Layout B, one slot per case of cases_b()."""
    p0, p1, w, _, _ = mc.cases_b()
    feats, n_groups, groups = mc.layout_b()
    eng = Engine(feats, n_groups, n_slots=p0.size)
    eng.load_state(0, groups, w[0][None, :], probs=[mc.probs_a(p0[0], True), mc.probs_a(p1[0], True)])
    pa = np.stack([mc.probs_a(x, (b & 1) == 0) for b, x in enumerate(p0)])
    pb = np.stack([mc.probs_a(x, (b & 2) == 0) for b, x in enumerate(p1)])
    for b in range(1, p0.size):
        eng.copy_slot(b, 0)
        eng.set_probs(b, 0, pa[b])
        eng.set_probs(b, 1, pb[b])
        eng.set_weights(b, w[b][None, :])
    return eng, p0.size


def run_cases():
    """Layout B through the matrix-pipe form under the current SBE_MFMA_SHARED; {name: (values, kernel name)} -- the protocol of
    tests/test_gpu_shared_epilogue.py's child-process helper, which runs this with SBE_MFMA_SHARED=0."""
    eng, n = _engine_b()
    with eng:
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        return {"b": (eng.mixture_loglik_batch(0, n), eng.last_mixture_kernel())}


# ---- reporting ----------------------------------------------------------------------------------------------------------
def _err(got, want):
    return np.abs(np.asarray(got, dtype=np.longdouble) - want).astype(np.float64)


def _ratio(err, bound):
    assert np.all(err[bound == 0] == 0)
    return np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)


def _report(tag, q, cls, row, err, bound):
    """One [mixlog] line per exponent class and per first / last / other table row: values compared, largest error / bound and
    where.  -> values compared per class."""
    ratio = _ratio(err, bound)
    seen = {}
    groups = [(f"class {name}", cls == k) for k, name in enumerate(mc.CLASSES)]
    groups += [("row 0", row == 0), ("row 1023", row == 1023), ("rows 1..1022", (row > 0) & (row < 1023))]
    for name, sel in groups:
        idx = np.flatnonzero(sel)
        if idx.size == 0:
            continue
        j = idx[np.argmax(ratio[idx])]
        seen[name.replace("class ", "")] = idx.size
        print(f"[mixlog] {tag} {name}: {idx.size} values, largest error / bound {ratio[j]:.3f} at {float(q[j]).hex()} (row {row[j]}): "
              f"error {err[j]:.3e}, bound {bound[j]:.3e}")
    return seen


def _worst(q, row, err, bound):
    ratio = _ratio(err, bound)
    j = int(np.argmax(ratio))
    return f"largest error / bound {ratio[j]:.3f} at {float(q[j]).hex()} (table row {row[j]}): error {err[j]:.3e}, bound {bound[j]:.3e}"


@pytest.fixture(scope="module")
def vals():
    return mc.values()


@pytest.fixture(scope="module")
def device_a(vals):
    """Layout A through the matrix-pipe form, once per N for the module: {N: (results, second launch)}."""
    cache = {}

    def get(N):
        if N not in cache:
            cache[N] = _run_a_mfma(N, vals[0])
        return cache[N]
    return get


def _class_counts(cls):
    return {name: int(np.sum(cls == k)) for k, name in enumerate(mc.CLASSES)}


# ---- the matrix-pipe form, one entry per state ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 1000])
def test_matrix_pipe_log_entry_by_entry(N, vals, device_a):
    """Layout A: LL[b] = N log q_b with ONE table entry -- count 1, count 3, and count 1000 over 16 k-blocks (the count-weighted
    exponent sum reaches 1000 x 874) -- within matrix_pipe_bound of np.longdouble for every generated value; a second launch
    returns the same bytes."""
    q, cls, row = vals
    got, again = device_a(N)
    d = q.astype(np.float64)
    assert np.all(np.isfinite(got))
    err, bound = _err(got, N * mc.log_ref(d)), mc.matrix_pipe_entry_bound(d, N)
    seen = _report(f"matrix pipe N={N}", q, cls, row, err, bound)
    counts = _class_counts(cls)
    assert {k: seen[k] for k in mc.CLASSES} == counts and sum(counts.values()) == q.size == got.size == 24391
    assert counts == {"half": 5116, "quarter": 5120, "2^-20": 5120, "min_normal": 5119, "subnormal": 3907, "named": 9}
    assert seen["row 0"] + seen["row 1023"] + seen["rows 1..1022"] == q.size
    assert np.all(err <= bound), _worst(q, row, err, bound)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize("N", [1, 3])
def test_matrix_pipe_log_equals_its_model_bit_for_bit(N, vals, device_a):
    """The device's result is the exact-arithmetic model's (tests/_mixlog_cases.py: the table as the host builds it, the index
    and exponent bits, five correctly rounded FMAs), carried through the kernel's end of lane -- lsum = fma(cnt, lg, 0), the
    integer exponent sum less 1023 x the column's objects, fma(K, ln2, lsum) once -- bit for bit.  Every step of that
    combination is restated exactly: in layout A everything else the block adds to a slot is an exact zero (entries
    without counts leave lsum as it is; the other lanes, waves and column splits hold 0.0)."""
    q, cls, row = vals
    got, _ = device_a(N)
    want = np.array([mc.model_ll(float(x), N) for x in q.astype(np.float64)])
    same = got.view(np.uint64) == want.view(np.uint64)
    print(f"[mixlog] matrix pipe N={N}: {int(same.sum())} of {q.size} values equal the model bit for bit")
    bad = np.flatnonzero(~same)
    assert bad.size == 0, [(float(q[j]).hex(), int(row[j]), got[j].hex(), want[j].hex()) for j in bad[:8]]


def test_log_of_one_and_of_a_half():
    one, half, below = np.float32(1.0), np.float32(0.5), np.nextafter(np.float32(1.0), np.float32(0.0))
    for N in (1, 1000):
        with _engine_a(N, 40) as eng:
            eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
            _set_a(eng, np.full(40, one), 0)
            got = _mfma_launch(eng, 40)
            assert np.all(got == 0.0), got                                      # log 1 = 0 exactly
            _set_a(eng, np.full(40, half), 0)
            got = _mfma_launch(eng, 40)
            # K = -N exactly and a mantissa part of exactly 0: one rounding of N x the kernel's ln 2, itself LN2_REL x 2^-53 off
            exact = -N * np.log(np.longdouble(2))
            assert np.all(_err(got, exact) <= (1 + mc.LN2_REL) * mc.U * float(-exact)), (got[0], float(exact))
            assert np.all(got == got[0])
            if N == 1:
                _set_a(eng, np.full(40, below), 0)
                got = _mfma_launch(eng, 40)
                want = mc.log_ref(np.float64(below))
                err = _err(got, want)
                print(f"[mixlog] log(nextafter(1, 0)) = {got[0]!r}: relative error {err.max() / float(-want):.3e}")
                assert np.all(err <= mc.matrix_pipe_entry_bound(np.float64(below), 1))
                assert np.all(err <= 1e-13 * float(-want))                     # the header comment's "log1p(-eps) to 1e-13 relative"


# ---- two entries: the shared-operand epilogue ------------------------------------------------------------------------------
def test_shared_operand_epilogue_entry_by_entry():
    """Layout B: LL[b] = n_both log(w0' p0 + w1' p1) + n_conf log p1 through the SHARE instance -- Dirichlet weights, a float32-
    subnormal cluster weight, a cluster weight of exactly 0 -- within the bound, and the same bytes from the per-entry epilogue
    (SBE_MFMA_SHARED=0, a fresh child process)."""
    from tests.test_gpu_shared_epilogue import _forced_old
    p0, p1, w, c0, c1 = mc.cases_b()
    got, name = run_cases()["b"]
    assert MFMA in name and "16 slots x M tiles 1, C=2, shared operands" in name, name
    v, cnt, want = mc.reference_b(p0, p1, w)
    assert got.size == p0.size == 3241 and np.all(np.isfinite(got))
    err, bound = _err(got, want), mc.matrix_pipe_state_bound(v, cnt, roundings_of_v=1)
    row = mc.interval_of(v[:, 0])
    for k, kind in enumerate(("Dirichlet weights", "subnormal cluster weight", "cluster weight 0")):
        sel = np.arange(p0.size) % 3 == k
        print(f"[mixlog] shared operands, {kind}: {int(sel.sum())} states, {_worst(v[sel, 0], row[sel], err[sel], bound[sel])}")
    _report("shared operands, p0 of", v[:, 0].astype(np.float64), c0, row, err, bound)
    assert np.all(err <= bound), _worst(v[:, 0], row, err, bound)
    old, old_name = _forced_old(__file__)["b"]
    assert MFMA in old_name and "shared operands" not in old_name and "16 slots x M tiles 1, C=2>" in old_name, old_name
    assert np.array_equal(got.view(np.uint64), old.view(np.uint64)), np.flatnonzero(got.view(np.uint64) != old.view(np.uint64))[:10]


# ---- one entry per tuple: the wide forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sl", sorted(mc.C_WIDTHS))
def test_wide_forms_with_far_apart_exponents(sl):
    """Layout C: every one of up to 28 (4 slots per block) / 64 (2 slots per block) tuples is occupied and has its own v_t, with
    exponents from 2^-149 to 2^0 in tuples that share an M tile's lane halves: the two halves' integer exponent sums are added
    before the bias leaves.  Also against k_mixture_tuple64 on the same states (it applies at both widths; asserted)."""
    n_groups = mc.C_WIDTHS[sl]
    feats, groups, tid, digits = mc.layout_c(n_groups)
    probs, weights = mc.cases_c(n_groups)
    v, cnt, want = mc.reference_c(n_groups, probs, weights, orc.normalize_weights)
    B, C = mc.C_SLOTS, len(n_groups)
    assert v.shape == (B, digits.shape[0]) and np.all(cnt > 0)
    with Engine(feats, n_groups, n_slots=B) as eng:
        for b in range(B):
            tables = []
            for c, g in enumerate(n_groups):
                p = np.zeros((g, 1, 2), dtype=np.float32)
                p[:, 0, 0] = probs[c][b]
                p[:, 0, 1] = (np.float32(1.0) - probs[c][b]) if b & 1 else 0.0
                tables.append(p)
            eng.load_state(b, groups, weights[b][None, :], probs=tables)
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        got = _mfma_launch(eng, B, f"{sl} slots x M tiles {-(-digits.shape[0] // (32 // sl))}, C={C}")
        assert np.array_equal(_mfma_launch(eng, B).view(np.uint64), got.view(np.uint64))
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE)
        other = eng.mixture_loglik_batch(0, B)                      # (one feature, two states: 64-feature tiles, the packed stream)
        other_name = eng.last_mixture_kernel()
        assert "k_mixture_tuple64" in other_name, other_name
    assert np.all(np.isfinite(got))
    err, bound = _err(got, want), mc.matrix_pipe_state_bound(v, cnt, roundings_of_v=C - 1, wide=True)
    spread = np.log2(v.max(-1) / v.min(-1))
    j = int(np.argmax(_ratio(err, bound)))
    print(f"[mixlog] wide form {sl} slots per block: {B} states x {v.shape[1]} tuples, exponent spread in a state {spread.min():.0f} .. "
          f"{spread.max():.0f} bits, largest error / bound {_ratio(err, bound)[j]:.3f} (state {j}: error {err[j]:.3e}, bound {bound[j]:.3e})")
    assert spread.max() > 120
    assert np.all(err <= bound), (j, err[j], bound[j])
    np.testing.assert_allclose(other, got, rtol=1e-12)
    print(f"[mixlog] wide form {sl} slots per block against {other_name.split('<')[0]}: "
          f"largest relative difference {np.max(np.abs(other - got) / np.abs(got)):.3e}")


# ---- every vector-pipe form over the exponent range ---------------------------------------------------------------------------
def _sweep_forms(eng, n, tag, want, bound_per_obs, n_obs, q, row, cls=None):
    """Every vector-pipe form in both log modes over the engine's n states, VECTOR_BATCH states per launch.  `bound_per_obs`:
    kernel name -> bound for LOG_PER_OBS when a state is ONE log (else None: the fuzzer's tolerance).  -> forms that ran."""
    ran = []
    for fname, kernel in VECTOR_FORMS.items():
        for mode, mname in ((LOG_PER_OBS, "LOG_PER_OBS"), (LOG_PRODUCT, "LOG_PRODUCT")):
            eng.set_option(kernel=kernel, log_mode=mode)
            got = np.empty(n)
            try:
                for lo in range(0, n, VECTOR_BATCH):
                    m = min(VECTOR_BATCH, n - lo)
                    got[lo:lo + m] = eng.mixture_loglik_batch(lo, m)
            except EngineError as exc:
                assert "not applicable" in str(exc), (fname, exc)
                print(f"[mixlog] {tag} {fname} {mname}: not applicable to this layout")
                continue
            name = eng.last_mixture_kernel()
            assert MFMA not in name, name
            one_log = bound_per_obs is not None and mode == LOG_PER_OBS
            bound = bound_per_obs(name) if one_log else mc.fuzz_tolerance(want.astype(np.float64), n_obs)
            err = _err(got, want)
            print(f"[mixlog] {tag} {fname} {mname} ({name.split('<')[0]}; {'per-log bound' if one_log else 'fuzzer tolerance'}): "
                  f"{n} states, {_worst(q, row, err, bound)}")
            assert np.all(np.isfinite(got)), (fname, mname)
            assert np.all(err <= bound), (fname, mname, _worst(q, row, err, bound))
            if cls is not None and mode == LOG_PRODUCT:
                sub = cls == mc.CLASSES.index("subnormal")                     # the running product strips 4 x (-149 ..) per step
                assert sub.sum() >= 500 and np.all(np.isfinite(got[sub])) and np.all(err[sub] <= bound[sub])
            ran.append((fname, mname))
    eng.set_option(kernel=MIXTURE_PACKED, log_mode=LOG_PER_OBS)
    return ran


@pytest.mark.parametrize("layout", ["A1", "A1000", "B"])
def test_every_form_over_the_exponent_range(layout):
    """The seven vector-pipe forms in both log modes on the strided value subset (every 8th table row of the matrix-pipe log,
    the first and last two and both sides of the split; all five mantissas, all five exponent classes, the named values):
    fast_log, the 128-row table log of k_mixture_tuple64 and the ProdAcc running product at exponents down to 2^-149.
    One log per state (layout A, N = 1, LOG_PER_OBS) is held to the project's per-log bounds; LOG_PRODUCT and N > 1 to the
    fuzzer's tolerance.  A form that answers "not applicable" is left out for that layout only; at least three forms run."""
    if layout == "B":
        p0, p1, w, c0, _ = mc.cases_b()
        v, cnt, want = mc.reference_b(p0, p1, w)
        eng, n = _engine_b()
        with eng:
            ran = _sweep_forms(eng, n, "layout B", want, None, mc.B_N, v[:, 0], mc.interval_of(v[:, 0]))
    else:
        N = int(layout[1:])
        q, cls, row = mc.values(mc.SUBSET_INTERVALS)
        d = q.astype(np.float64)
        assert q.size == 3241 and _class_counts(cls) == {"half": 661, "quarter": 665, "2^-20": 665, "min_normal": 664, "subnormal": 577, "named": 9}
        want = N * mc.log_ref(d)
        per_obs = (lambda name: mc.per_obs_bound(want.astype(np.float64), name)) if N == 1 else None
        with _engine_a(N, q.size) as eng:
            _set_a(eng, q, 0)
            ran = _sweep_forms(eng, q.size, f"layout A N={N}", want, per_obs, N, q, row, cls)
    forms = {f for f, _ in ran}
    assert len(forms) >= 3, ran
    assert all((f, "LOG_PER_OBS") in ran and (f, "LOG_PRODUCT") in ran for f in forms), ran


# ---- the 32-bit exponent sums next to their guard -----------------------------------------------------------------------------
def test_exponent_sums_close_under_the_overflow_guard(monkeypatch):
    """mfma_geometry refuses a launch when passes x 2 x N x 2100 >= 2^31 (a lane's biased exponent sum per slot, 32 bits).
    N is bounded by the A image in LDS: one M tile of 4 slots x 8 tuples over KBp k-blocks of 64 objects is KBp KB next to the
    16 KB log table and 2.3 KB of metadata and reduction scratch in 160 KB, so KBp <= 140, N <= 8960.  With N = 8900 the guard
    admits 57 passes (a pass is 16 column tiles of 32 columns) in ONE column split (SBE_MFMA_SPLIT=1) and refuses 58: this is
    the 57-pass geometry, 0.8 % under the limit.  The guard's worst case is a lane whose columns each hold all N objects: here
    S = 2 and every object observes state 0 of every feature, so every even column (an even lane's two columns per pass) holds N
    objects.  The sum a lane reaches is computed below from the column counts and asserted: 114 columns x 8900 x 1023 = 1.04e9
    (0.48 x 2^31) in the state with every v in [0.7072, 1) (biased exponent 1023, the largest a probability has), and
    114 x 8900 x 874 in the state with every v = 2^-149, whose sum after the bias leaves is the most negative.
    Reference: with one observed state per feature the oracle's composition is LL = sum_g n_g sum_f log p[g, f, 0]; it is
    taken in np.longdouble from the tables and tied to the oracle's own functions on the first features (the whole block
    through the oracle is 8900 x 14 560 x 2 products twice over).  Tolerance: the fuzzer's.
    Control: the same objects with 58 passes' worth of columns are refused while the single split is forced -- which shows
    that the setting took effect, a 57-way split being one pass per block -- and accepted without it."""
    N, F, S, G = 8900, 14560, 2, 4
    F_control = 14593

    def geometry(f):                                  # (column tiles, passes of 16 tiles in one split: mfma_geometry)
        nt = -(-f * S // 32)
        return nt, -(-(nt + nt % 2) // 16)

    NT, passes = geometry(F)
    assert passes == 57 and geometry(F_control)[1] == 58 and passes * 2 * N * 2100 < 2 ** 31 <= (passes + 1) * 2 * N * 2100
    assert -(-N // 64) <= 140
    # what a lane's 32-bit sum reaches: wave w takes the tiles 2 w + r + 16 pass (r = 0, 1), lane l their columns 32 tile + l
    colcount = np.zeros((NT + 16) * 32, dtype=np.int64)
    colcount[0:F * S:2] = N
    per_lane = np.array([[sum(int(colcount[t * 32 + lane]) for pa in range(passes) for t in (2 * w + 16 * pa, 2 * w + 1 + 16 * pa))
                          for lane in range(32)] for w in range(8)])
    reached = int(per_lane.max()) * 1023
    print(f"[mixlog] exponent sums: a lane counts up to {per_lane.max()} objects over {passes} passes; biased sum {reached} = "
          f"{reached / 2.0 ** 31:.3f} x 2^31 (v in [0.7072, 1)), {int(per_lane.max()) * 874} (v = 2^-149)")
    assert per_lane.max() == 2 * passes * N and 2 ** 31 // 4 <= reached < 2 ** 31
    monkeypatch.setenv("SBE_MFMA_SPLIT", "1")
    rng = np.random.default_rng(mc.SEED + 9)
    big = np.zeros((N, F_control, S), dtype=bool)
    big[:, :, 0] = True
    gid = np.arange(N) % G
    groups = [np.stack([gid == k for k in range(G)])]
    n_g = np.bincount(gid, minlength=G).astype(np.longdouble)
    near_one = np.empty((G, F_control, S), dtype=np.float32)
    near_one[..., 0] = np.float32(0.7072) + np.float32(0.2927) * rng.random((G, F_control), dtype=np.float32)
    near_one[..., 1] = np.float32(1.0) - near_one[..., 0]
    assert near_one[..., 0].min() >= 0.7072 and near_one[..., 0].max() < 1.0
    smallest = np.full((G, F_control, S), 2.0 ** -149, dtype=np.float32)

    def reference(p, n_feat):
        return float((n_g[:, None] * mc.log_ref(p[:, :n_feat, 0].astype(np.float64))).sum())

    for p in (near_one, smallest):                                                 # the restatement is the oracle's, on 8 features
        f8 = np.ascontiguousarray(big[:, :8])
        lh = np.empty((N, 8, 1))
        orc.compute_component_likelihood(f8, p[:, :8], groups[0], np.arange(G), lh[..., 0])
        w = orc.normalize_weights(np.ones((8, 1), dtype=np.float32), orc.has_components(groups))
        assert np.log(orc.mixture_observation_lh(w, lh)).sum() == pytest.approx(reference(p, 8), rel=1e-13)
    want = np.array([reference(near_one, F), reference(smallest, F)])
    assert want[1] == pytest.approx(N * F * -149 * np.log(2.0), rel=1e-14)
    with Engine(big, [G], n_slots=1) as eng:                                       # the control: one pass more
        eng.load_state(0, groups, np.ones((F_control, 1), dtype=np.float32), probs=[near_one])
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        with pytest.raises(EngineError, match="not applicable"):
            eng.mixture_loglik_batch(0, 1)
        monkeypatch.delenv("SBE_MFMA_SPLIT")
        split = _mfma_launch(eng, 1, "4 slots x M tiles 1, C=1")
        assert abs(split[0] - reference(near_one, F_control)) <= mc.fuzz_tolerance(reference(near_one, F_control), N * F_control)
        monkeypatch.setenv("SBE_MFMA_SPLIT", "1")
    feats = np.ascontiguousarray(big[:, :F])
    del big
    with Engine(feats, [G], n_slots=2) as eng:
        for b, p in enumerate((near_one, smallest)):
            eng.load_state(b, groups, np.ones((F, 1), dtype=np.float32), probs=[np.ascontiguousarray(p[:, :F])])
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        got = _mfma_launch(eng, 2, "4 slots x M tiles 1, C=1")
    tol = mc.fuzz_tolerance(want, N * F)
    print(f"[mixlog] exponent sums at {passes} passes x 2 x {N} objects: relative error {np.abs(got - want) / np.abs(want)} (tolerance 1e-10)")
    assert np.all(np.abs(got - want) <= tol), (got, want)
