"""The range cases of the collapsed likelihood's per-feature term (the Dirichlet-categorical log-pdf: k_dcl<float> and
k_dcl<int32_t>, collapsed_group_block, the tile blocks of step_core_body), shared by tests/test_collapsed_range_cpu.py (the
oracle and three wrong restatements under the checker) and tests/test_gpu_collapsed_range.py (the device).  DESIGN.md 4.2.

Reference.  mpmath at 40 digits on the arguments exactly as the kernels form them, which the host reproduces bit for bit:

    n   = the float32 NumPy-order sum of the row's float32 counts        np.sum(c, dtype=np.float32)
    A   = the float64 NumPy-order sum of the row's concentrations        np.sum(a)
    x1  = fl64(float64(n) + A)
    y_s = fl64(float64(c_s) + a_s)                                       for every state with a_s > 0
    E   = lgamma(A) - lgamma(x1) + sum_{a_s > 0} (lgamma(y_s) - lgamma(a_s))

A state with a_s == 0 is not applicable and contributes nothing, whatever its count (its count is still part of n).

Bound.  Derived, nothing in it is tuned.  M = the sum over the 2 + 2 S+ lgamma values above of max(1, |value|);
B = (EPS_L + k u) M with EPS_L = 1e-14 the documented error of sbe_lgamma_pos (relative to max(1, |lgamma|); pinned by
test_gpu_engine.py::test_lgamma_accuracy), u = 2^-53 and k = k_of(S) the float64 additions a term passes through:

    k_of(S) = depth(S) + 3      depth(n) = n                                     for n < 8     (the chain 0 + a_0 + a_1 + ...)
                                         = (n // 8 - 1) + 3 + n % 8              for n <= 128  (8 accumulators, their tree, the tail)
                                         = 1 + max(depth(h), depth(n - h))       beyond, h = n // 2 - (n // 2) % 8

depth(n) is the most additions any element passes through in NumPy's pairwise sum of n elements; the 3 are the difference of
the state's pair, the difference of the row constant and the addition of constant and series.  The device's float32 value v
must satisfy |float64(v) - E| <= B + ulp32(|E| + B) / 2.  An entry is SHARP when B <= ulp32(|E|) / 8: there the inequality
says v == float32(E) unless E lies within B of a midpoint of two float32 numbers (`near_mid`).

Exact zeros.  Where the same function is differenced on the same arguments E is 0 exactly and the device must return +0.0:
a row whose counts are all zero (x1 == A, y_s == a_s), and a row with one applicable state alone and no count elsewhere
(A == a_s and x1 == y_s bit for bit; every row at S = 1).  Such rows (`zero`) are asserted equal and left out of the sharp share.

A case is one engine: S, F, and two components -- component 0 with a shared [F, S] concentration, component 1 with a
per-group [G, F, S] one, so that every stateless call runs both forms of k_dcl's concentration pointer and every resident
call of component 1 runs with g_lo != 0.  `case(name)` builds it once, `reference(name, c)` evaluates component c once."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import mpmath
import numpy as np

MP_DIGITS = 40
EPS_L = 1e-14
U = 2.0 ** -53
SHARP_CAP = 0.15                          # at most this share of a family's non-zero rows may be non-sharp
F32, F64 = np.float32, np.float64


# ---- NumPy's pairwise order ----------------------------------------------------------------------------------------------
def depth(n):
    if n < 8:
        return n
    if n <= 128:
        return (n // 8 - 1) + 3 + n % 8
    h = n // 2 - (n // 2) % 8
    return 1 + max(depth(h), depth(n - h))


def k_of(s):
    return depth(s) + 3


def pairwise(a):
    """(sum, depth) of NumPy's pairwise_sum written out literally for the 1-D array `a`, in a's own dtype; the depth of
    a partial sum is one more than the deeper of its operands', an element's and the initial zero's is 0."""
    a = np.asarray(a)

    def add(x, y):
        return x[0] + y[0], 1 + max(x[1], y[1])

    def walk(lo, n):
        if n < 8:
            res = (a.dtype.type(0), 0)
            for i in range(n):
                res = add(res, (a[lo + i], 0))
            return res
        if n <= 128:
            r = [(a[lo + j], 0) for j in range(8)]
            lim = n - n % 8
            for i in range(8, lim, 8):
                for j in range(8):
                    r[j] = add(r[j], (a[lo + i + j], 0))
            res = add(add(add(r[0], r[1]), add(r[2], r[3])), add(add(r[4], r[5]), add(r[6], r[7])))
            for i in range(lim, n):
                res = add(res, (a[lo + i], 0))
            return res
        h = n // 2
        h -= h % 8
        return add(walk(lo, h), walk(lo + h, n - h))

    return walk(0, len(a))


def ulp32(x):
    """The spacing of float32 at |x| (float64 in, float64 out; 2^-149 below the normal range)."""
    x = np.abs(np.asarray(x, dtype=F64))
    _m, e = np.frexp(x)
    return np.where(x < 2.0 ** -126, 2.0 ** -149, np.ldexp(1.0, e - 24))


# ---- the exact reference ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lgamma(x):
    return mpmath.loggamma(mpmath.mpf(x))


def exact(counts, conc):
    """The reference of float32 counts [G, F, S] under conc [F, S] or [G, F, S]: float64 arrays [G, F] E_hi + E_lo (the
    40-digit E as a double and its remainder), M, B, r32 (float32(E)), and the masks zero / zero_counts / sharp / near_mid."""
    counts = np.ascontiguousarray(counts, dtype=F32)
    conc = np.ascontiguousarray(conc, dtype=F64)
    G, F, S = counts.shape
    k = k_of(S)
    e_hi, e_lo, m_sum = np.zeros((G, F)), np.zeros((G, F)), np.zeros((G, F))
    zero = np.zeros((G, F), dtype=bool)
    with mpmath.workdps(MP_DIGITS):
        for g in range(G):
            for f in range(F):
                c, a = counts[g, f], (conc[f] if conc.ndim == 2 else conc[g, f])
                n = np.sum(c, dtype=F32)
                big_a = np.sum(a)
                x1 = F64(n) + big_a
                y = c.astype(F64) + a
                vals = [_lgamma(float(big_a)), _lgamma(float(x1))]
                total = vals[0] - vals[1]
                for s in np.flatnonzero(a > 0):
                    ly, la = _lgamma(float(y[s])), _lgamma(float(a[s]))
                    total += ly - la
                    vals += [ly, la]
                hi = float(total)
                e_hi[g, f], e_lo[g, f] = hi, float(total - mpmath.mpf(hi))
                m_sum[g, f] = float(sum(max(mpmath.mpf(1), abs(v)) for v in vals))
                zero[g, f] = total == 0
    b = (EPS_L + k * U) * m_sum
    r32 = e_hi.astype(F32)
    # the float32 neighbour of r32 on E's side, and the midpoint between them (exact in float64)
    above = (F64(r32) - e_hi) - e_lo > 0                                       # r32 > E: the other neighbour lies below
    other = np.where(above, np.nextafter(r32, F32(-np.inf)), np.nextafter(r32, F32(np.inf)))
    mid = 0.5 * (F64(r32) + F64(other))
    near_mid = np.abs((mid - e_hi) - e_lo) <= b
    return SimpleNamespace(E_hi=e_hi, E_lo=e_lo, M=m_sum, B=b, r32=r32, zero=zero, zero_counts=~counts.any(axis=-1),
                           sharp=~zero & (b <= ulp32(e_hi) / 8), near_mid=near_mid, k=k)


def check(ref, v):
    """The device's (or the oracle's) float32 [G, F] against the reference: err = |float64(v) - E|, the bound, and the
    entries that meet it / are +0.0 where E is exactly 0 / equal float32(E) where the contract says they must."""
    v = np.asarray(v)
    assert v.dtype == F32 and v.shape == ref.B.shape
    err = np.abs((v.astype(F64) - ref.E_hi) - ref.E_lo)
    bound = ref.B + 0.5 * ulp32(np.abs(ref.E_hi) + ref.B)
    must_equal = ref.sharp & ~ref.near_mid
    live = ~ref.zero
    return SimpleNamespace(err=err, bound=bound, within=err <= bound, plus_zero=v.view(np.uint32) == 0,
                           bit_equal=v.view(np.uint32) == ref.r32.view(np.uint32), must_equal=must_equal,
                           worst=float(np.max(err[live] / bound[live], initial=0.0)),
                           equal_share=float(np.mean(v.view(np.uint32)[live] == ref.r32.view(np.uint32)[live])) if live.any() else 1.0,
                           sharp_share=float(np.mean(ref.sharp[live])) if live.any() else 1.0)


def assert_meets(ref, v, what):
    """The contract on v; returns check(ref, v) for the caller's printed line."""
    r = check(ref, v)
    assert r.plus_zero[ref.zero].all(), (what, "an exactly-zero row is not +0.0", np.argwhere(ref.zero & ~r.plus_zero).tolist()[:8])
    assert r.within.all(), (what, "outside the bound", [(g, f, float(r.err[g, f]), float(r.bound[g, f])) for g, f in np.argwhere(~r.within)[:8]])
    bad = r.must_equal & ~r.bit_equal
    assert not bad.any(), (what, "a sharp entry away from a midpoint is not float32(E)", np.argwhere(bad).tolist()[:8])
    return r


def line(what, r):
    return f"[collapsed-range] {what}: worst |v - E| / bound {r.worst:.3f}, bit-equal to float32(E) {r.equal_share:.1%}, sharp {r.sharp_share:.1%}"


# ---- building blocks --------------------------------------------------------------------------------------------------
def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def moderate_conc(rng, shape):
    """[.., F, S]: feature f is log-uniform in [1e-3, 50] (f % 4 == 0), all 1 (1), all 0.5 (2) or all 1 / S (3)."""
    a = log_uniform(rng, 1e-3, 50.0, shape)
    s = shape[-1]
    for kind, value in ((1, 1.0), (2, 0.5), (3, 1.0 / s)):
        a[..., kind::4, :] = value
    return a


def extreme_conc(rng, shape):
    return log_uniform(rng, 1e-6, 1e4, shape)


def counts_below(rng, levels, g0, g, f, s):
    """float32 [g, f, s]: row (i, j) draws integers below levels[(g0 + i + j // 4) % len(levels)]; row (0, 0) is all zero."""
    top = np.array(levels)[(g0 + np.arange(g)[:, None] + np.arange(f)[None, :] // 4) % len(levels)]
    c = np.floor(rng.random((g, f, s)) * top[:, :, None]).astype(F32)
    c[0, 0] = 0
    return c


def build(name, family, seed, s, f, groups, conc_of, levels, finish=None):
    rng = np.random.default_rng(seed)
    conc = [np.ascontiguousarray(conc_of(rng, (f, s))), np.ascontiguousarray(conc_of(rng, (groups[1], f, s)))]
    counts = [counts_below(rng, levels, 0, groups[0], f, s), counts_below(rng, levels, groups[0], groups[1], f, s)]
    if finish is not None:
        finish(rng, counts, conc)
    n_obj = 12
    feats = np.eye(s, dtype=bool)[rng.integers(0, s, size=(n_obj, f))]
    for arr in counts + conc + [feats]:
        arr.setflags(write=False)
    return SimpleNamespace(name=name, family=family, S=s, F=f, n_groups=list(groups), counts=counts, conc=conc, features=feats)


def mask_states(rng, counts, conc):
    """About 15 % of the states become not applicable (a = 0); every row keeps a positive state."""
    for a in conc:
        dead = rng.random(a.shape) < 0.15
        dead[..., 0] &= ~dead.all(axis=-1)
        a[dead] = 0.0


F32N_BIG = (2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 25 + 4)
F32N_ODD = (1, 3, 5, 7, 9)


def f32_totals(rng, counts, conc):
    """Every row: one state at 2^24 or just above (an exact float32 integer), up to five odd counts below 10 on others, zeros
    elsewhere -- the integer sum of most rows is no float32, and at S >= 9 the float32 sum depends on NumPy's order."""
    for c in counts:
        g, f, s = c.shape
        c[...] = 0
        for i in range(g):
            for j in range(f):
                where = rng.permutation(s)
                if i == j == 0:
                    continue                                                           # (the all-zero row stays)
                c[i, j, where[0]] = F32N_BIG[(i + j) % len(F32N_BIG)]
                for pos in where[1:1 + min(s - 1, 1 + (i + j) % 5)]:
                    c[i, j, pos] = rng.choice(F32N_ODD)


def sparse_counts(rng, counts, conc):
    """254 states, most of them unobserved: seven in ten counts are 0."""
    for c in counts:
        c[rng.random(c.shape) < 0.7] = 0


EDGE_S = (1, 2, 7, 8, 9, 16, 17, 128, 129, 254)
MODERATE_LEVELS, EXTREME_LEVELS = (2, 30, 300, 3000), (2, 100, 60000)

CASES = {}
for _s in EDGE_S:
    CASES[f"edges_S{_s}"] = functools.partial(build, f"edges_S{_s}", "S edges", 100 + _s, _s, 12, (2, 2), moderate_conc, MODERATE_LEVELS)
for _s in (4, 20):
    CASES[f"moderate_S{_s}"] = functools.partial(build, f"moderate_S{_s}", "moderate", 200 + _s, _s, 48, (3, 3), moderate_conc, MODERATE_LEVELS)
for _s in (3, 12, 40):
    CASES[f"extreme_S{_s}"] = functools.partial(build, f"extreme_S{_s}", "extreme", 300 + _s, _s, 48, (3, 3), extreme_conc, EXTREME_LEVELS)
for _s in (6, 40):
    CASES[f"masked_S{_s}"] = functools.partial(build, f"masked_S{_s}", "masked", 400 + _s, _s, 24, (2, 3), moderate_conc, (30,), mask_states)
for _s in (2, 9, 130):
    CASES[f"f32n_S{_s}"] = functools.partial(build, f"f32n_S{_s}", "float32 n", 500 + _s, _s, 16, (2, 2), moderate_conc, (1,), f32_totals)
for _f in (48, 49):                       # 48 * 254 * 8 + 48 * 4 = 97 728 <= 96 KB = 98 304 < 99 764 = 49 * 254 * 8 + 49 * 4
    CASES[f"lds_F{_f}"] = functools.partial(build, f"lds_F{_f}", "LDS switch", 600 + _f, 254, _f, (1, 1), moderate_conc, (300,), sparse_counts)

FAMILIES = {}
for _name, _make in CASES.items():
    FAMILIES.setdefault(_make.args[1], []).append(_name)
UNCAPPED = ("float32 n",)                 # 2^24 under every row: M is near 1e9 and no entry is sharp; the bound itself still sees one count


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def reference(name, component):
    c = case(name)
    return exact(c.counts[component], c.conc[component])


def group_sums(pf):
    """float64 [G]: NumPy's float32 sum of every row of the float32 [G, F] per-feature values, as the per-group cache holds it."""
    return np.array([F64(row.sum()) for row in np.asarray(pf, dtype=F32)])


# ---- the one-call step: counts come from the objects, so a small state of its own --------------------------------------------
STEP_N, STEP_F, STEP_S, STEP_G = 40, 24, 5, 3


@functools.lru_cache(maxsize=None)
def step_state(kind):
    """A state for Engine.step at the range's concentrations (`kind`: "moderate" or "extreme"): STEP_G disjoint clusters and
    one confounder group over STEP_N objects, every observation's source the cluster effect where the object is in a
    cluster, the confounder elsewhere; the change flips the source of objects 0 and 1."""
    rng = np.random.default_rng({"moderate": 701, "extreme": 702}[kind])
    conc_of = {"moderate": moderate_conc, "extreme": extreme_conc}[kind]
    n, f, s, g = STEP_N, STEP_F, STEP_S, STEP_G
    feats = np.eye(s, dtype=bool)[rng.integers(0, s, size=(n, f))]
    gid = rng.integers(0, g + 1, size=n)
    gid[:2] = 0
    groups = [np.stack([gid == i for i in range(g)]), np.ones((1, n), dtype=bool)]
    src = np.zeros((n, f, 2), dtype=bool)
    src[..., 0] = groups[0].any(axis=0)[:, None]
    src[..., 1] = ~src[..., 0]
    changed = np.array([0, 1], dtype=np.int32)
    return SimpleNamespace(features=feats, groups=groups, source=src, changed=changed, rows=~src[changed], n_groups=[g, 1],
                           conc=[conc_of(rng, (f, s)), conc_of(rng, (1, f, s))], weights=np.full((f, 2), 0.5, dtype=F32))
