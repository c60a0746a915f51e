"""The exact-arithmetic model of the matrix-pipe kernel's table log (tests/_mixlog_cases.py: fine_table, model_tab_log,
model_ll) against mpmath at 200 bits, over every generated value: the derived bound holds on paper and is honest (within
eight times the model's largest error), np.longdouble's log is good enough to stand in for mpmath on the device, and the
generator covers what it says.  No device."""
import numpy as np
import pytest

from tests import _mixlog_cases as mc

COUNTS = (1, 3, 1000)


@pytest.fixture(scope="module")
def vals():
    return mc.values()


@pytest.fixture(scope="module")
def truth(vals):
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    return mp, [mp.log(mp.mpf(float(x))) for x in vals[0]]


@pytest.fixture(scope="module")
def model(vals):
    return [mc.model_tab_log(float(x)) for x in vals[0]]


def test_generator_covers_every_interval_class_and_named_value(vals):
    q, cls, row = vals
    assert q.dtype == np.float32 and np.unique(q.view(np.uint32)).size == q.size
    d = q.astype(np.float64)
    assert np.all(d >= np.finfo(np.float64).tiny) and np.all(np.isfinite(np.log(d)))       # positive normal doubles
    named = mc.named_values()
    n_named = len(named)
    assert n_named == 9 and np.array_equal(q[:n_named], np.array([v for _, v in named], dtype=np.float32))
    assert np.all(cls[:n_named] == mc.CLASSES.index("named"))
    count = {name: int(np.sum(cls == k)) for k, name in enumerate(mc.CLASSES)}
    # 1024 intervals x 5 mantissas per class; the grid loses what a named value already is: 0.5 and both neighbours of the split
    # in [0.5, 1) (the split's successor is a lower edge's successor, its predecessor an upper edge's), nextafter(1, 0) (the last upper edge's
    # predecessor), 2^-126 among the normals
    assert count == {"half": 5120 - 4, "quarter": 5120, "2^-20": 5120, "min_normal": 5120 - 1,
                     "subnormal": count["subnormal"], "named": 9}, count
    assert count["subnormal"] == 3907                              # truncated mantissas collapse: what is left of 5120
    for k, name in enumerate(mc.CLASSES[:5]):
        sel = cls == k
        assert np.array_equal(np.unique(row[sel]), np.arange(1024)), name          # every interval in every class
        lo, hi = {"half": (0.5, 1.0), "quarter": (0.25, 0.5), "2^-20": (2.0 ** -20, 2.0 ** -19),
                  "min_normal": (2.0 ** -126, 2.0 ** -125), "subnormal": (2.0 ** -149, 2.0 ** -126)}[name]
        assert np.all(d[sel] >= lo) and np.all(d[sel] < hi), name
    sub = d[cls == mc.CLASSES.index("subnormal")]
    # every subnormal binade 2^-127 .. 2^-148; the last one holds 2^-149 alone, which is a named value
    assert np.array_equal(np.unique(np.floor(np.log2(sub))), np.arange(-148.0, -126.0))
    # the five mantissas of an interval, in the normal classes: both edges' neighbours exactly
    h = q[cls == 1].view(np.uint32) & np.uint32(0x7FFFFF)
    for i in (0, 1, 423, 424, 1023):
        inside = {int(x) for x in h[(h >> 13) == i]}
        lo = i << 13
        assert len(inside) == 5 and {lo, lo + 1, lo + (1 << 12), lo + (1 << 13) - 1} <= inside, i
    # the subset used by the layouts with several values per state keeps the same structure
    qs, cs, rs = mc.values(mc.SUBSET_INTERVALS)
    assert qs.size <= 4096 and set(np.unique(rs)) >= set(mc.SUBSET_INTERVALS)
    assert {0, 1, mc.SPLIT - 1, mc.SPLIT, 1022, 1023} <= set(mc.SUBSET_INTERVALS)
    assert np.all(np.isin(qs.view(np.uint32), q.view(np.uint32)))


def test_table_and_log_of_one(vals):
    tab = mc.fine_table()
    assert tab[0, 1] == 0.0 and tab[1023, 1] == 0.0 and tab[0, 0] == 0.5 and tab[1023, 0] == 0.25
    assert mc.model_tab_log(1.0) == (0.0, mc.BIAS)
    for n in COUNTS:
        assert mc.model_ll(1.0, n) == 0.0
    # rows below the split hold log c > 0, rows from it on log(c / 2) < 0, and the carry flips the exponent exactly there
    assert np.all(tab[1:mc.SPLIT, 1] > 0) and np.all(tab[mc.SPLIT:1023, 1] < 0)
    edge = 1.0 + mc.SPLIT / 1024.0
    assert mc.model_tab_log(np.nextafter(edge, 0.0))[1] == mc.BIAS and mc.model_tab_log(edge)[1] == mc.BIAS + 1
    assert np.log(edge) < np.log(2.0) / 2 < -np.log(edge / 2)       # the no-cancellation argument of matrix_pipe_bound


def test_ln2_constant(truth):
    mp, _ = truth
    rel = abs(mp.mpf(mc.LN2_D) - mp.log(2)) / mp.log(2) / mp.mpf(2) ** -53
    assert rel <= mc.LN2_REL, rel


def test_longdouble_log_agrees_with_mpmath(vals, truth):
    mp, logs = truth
    got = mc.log_ref(vals[0].astype(np.float64))
    assert np.finfo(np.longdouble).nmant >= 63
    worst = 0.0
    for x, g, t in zip(vals[0], got, logs):
        if t == 0:
            assert g == 0
            continue
        # a longdouble -> mpf without going through a double: high and low part
        hi = float(g)
        lo = float(g - np.longdouble(hi))
        worst = max(worst, float(abs((mp.mpf(hi) + mp.mpf(lo)) - t) / abs(t)))
    print(f"[mixlog] np.longdouble log against mpmath: largest relative error {worst:.3e} (2^-60 = {2.0 ** -60:.3e})")
    assert worst <= 2.0 ** -60


def test_model_within_the_matrix_pipe_bound_and_bound_honest(vals, truth, model):
    q, cls, row = vals
    mp, logs = truth
    d = q.astype(np.float64)
    overall = 0.0
    for n in COUNTS:
        bound = mc.matrix_pipe_entry_bound(d, n)
        err = np.array([float(abs(mp.mpf(mc.model_combine(lg, k, n)) - n * t)) for (lg, k), t in zip(model, logs)])
        assert bound.shape == err.shape
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
        assert np.all(err[bound == 0] == 0)                       # log 1
        for k, name in enumerate(mc.CLASSES):
            sel = np.flatnonzero(cls == k)
            j = sel[np.argmax(ratio[sel])]
            rel = err[j] / abs(float(logs[j]) * n) if logs[j] != 0 else 0.0
            print(f"[mixlog] model n={n} class {name}: {sel.size} values, largest error / bound {ratio[j]:.3f} at q={float(q[j]).hex()} "
                  f"(row {row[j]}), error {err[j]:.3e} = {rel:.3e} relative")
        assert ratio.max() <= 1.0, (n, ratio.max(), float(q[ratio.argmax()]).hex())
        overall = max(overall, ratio.max())
        away = err[(d < 1 - 2.0 ** -10)] / np.abs(n * np.log(d[d < 1 - 2.0 ** -10]))
        print(f"[mixlog] model n={n}: largest relative error away from 1: {away.max():.3e} ({away.max() / mc.U:.2f} x 2^-53)")
    # the derived constants are honest: the bound is below eight times the model's largest error somewhere
    assert overall > 1.0 / 8.0, overall


def test_multi_entry_reference_restatements():
    """normalized_pair is the oracle's float32 normalisation; layout C's tuple ids cover every tuple."""
    from oracle import sbayes_oracle as orc
    p0, p1, w, _, _ = mc.cases_b()
    assert p0.size <= 4096 and np.count_nonzero(w[:, 0] == 0) >= p0.size // 3 and np.all(w[:, 1] > 0)
    tiny = np.finfo(np.float32).tiny
    assert np.count_nonzero((w[:, 0] > 0) & (w[:, 0] < tiny)) >= p0.size // 3
    mine = mc.normalized_pair(w)
    for b in range(0, p0.size, 97):
        want = orc.normalize_weights(w[b][None, :], np.array([[True, True], [False, True]]))
        assert np.array_equal(want[0, 0], mine[b]) and np.array_equal(want[1, 0], np.array([0, 1], dtype=np.float32))
    v, cnt, ll = mc.reference_b(p0, p1, w)
    assert np.all(v > 0) and np.all(v <= 1) and np.all(np.isfinite(ll.astype(np.float64)))
    assert np.array_equal(v[w[:, 0] == 0, 0], p1[w[:, 0] == 0].astype(np.float64))         # weight 0: v = p1 exactly
    for sl, n_groups in mc.C_WIDTHS.items():
        feats, groups, tid, digits = mc.layout_c(n_groups)
        KT = digits.shape[0]
        assert KT == {4: 28, 2: 64}[sl] and np.unique(tid).size == KT and len({tuple(r) for r in digits}) == KT
        assert orc.has_components(groups).shape == (mc.C_N, len(n_groups))
        assert np.array_equal(orc.has_components(groups), (digits >= 0)[tid])
        probs, weights = mc.cases_c(n_groups, 3)
        v, cnt, ll = mc.reference_c(n_groups, probs, weights, orc.normalize_weights)
        assert cnt.sum() == mc.C_N and np.all(cnt > 0) and np.all(v > 0) and np.all(v <= 1.0 + 1e-6)
        assert np.log2(v.max() / v.min()) > 100                     # far-apart exponents in one state
        # against the oracle's own composition
        na = ~feats.any(-1)
        for b in range(3):
            lh = np.empty((mc.C_N, 1, len(n_groups)))
            for c, g in enumerate(n_groups):
                p = np.zeros((g, 1, 2), dtype=np.float32)
                p[:, 0, 0] = probs[c][b]
                orc.compute_component_likelihood(feats, p, groups[c], np.arange(g), lh[..., c])
            wn = orc.normalize_weights(weights[b][None, :], orc.has_components(groups))
            want = np.log(orc.mixture_observation_lh(wn, lh))[~na].sum()
            assert abs(float(ll[b]) - want) <= 1e-12 * abs(want)
