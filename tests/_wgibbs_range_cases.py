"""The range cases of the Gibbs weights step (sbayes_amd/csrc/sbe_wgibbs.hip), shared by tests/test_wgibbs_range_cpu.py (which
asserts under tests/_wgibbs_oracle.py alone that every case covers what it is there for, that its decisions are safe and that
the oracle agrees with a 50-digit evaluation) and tests/test_gpu_wgibbs_range.py (device against oracle and against the
50-digit values).  Four groups, DESIGN.md section 15:

    A  weight magnitudes and the row sum: every C from 2 to 8, Dirichlet rows with one or two components overwritten by 0,
       float32 denormals and small normals, at i1, at i2, at another component and at both; patterns without i1, without i2,
       without both, and of one component alone (a normalising sum of 0 where that component's weight is 0).
    B  draws, priors and temperatures at their ends (a2 = 0 and 1, denormal a2, A = 1 and B = 1 exactly, alpha from 1e-3 to
       1e4 and exactly 1 on a zero weight, T from 1e-3 to 1e3, u = 0 and 1 - 2^-24), every feature built for one of the four
       classes of log_p: finite, NaN, +inf, -inf.
    C  decisions at close range: u the float32 neighbours of float32(p).
    D  shapes and places: N around the sweep of 512 objects, features all NA / observed at the last object only / of one
       source, 64 patterns over two feature tiles, F on either side of the tile, the last of three slots.

A case is a dict: the state (w, has_components, src, na), the proposal (i1, i2, a2, u, alpha, beta_ab, t), the oracle's result
(patterns, pid, w_new, a2_old, w_out, accept, terms, band, margin, cls) and, for groups B and C, what every feature was built
for.  `case(name)` computes it once; its arrays are read-only.  The generator REFUSES a state in which a feature with a finite
log_p decides within twice the device band of its uniform (`Refused`), as tests/golden/make_golden_wgibbs.py does: the GPU
test then excludes nothing."""
from __future__ import annotations

import functools
import itertools

import mpmath
import numpy as np

from tests import _wgibbs_oracle as worc
from tests.test_gpu_wgibbs import SWEEP, synthetic_state

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
MP_DIGITS = 50
F32 = np.float32


class Refused(ValueError):
    """A feature's uniform lies within twice the device band of its p."""


def classes(log_p):
    log_p = np.asarray(log_p)
    return np.where(np.isnan(log_p), NAN, np.where(log_p == np.inf, PINF, np.where(log_p == -np.inf, NINF, FINITE)))


def class_counts(cls):
    return tuple(int((np.asarray(cls) == k).sum()) for k in (FINITE, NAN, PINF, NINF))


STATE_KEYS = ("w", "has_components", "src", "na", "i1", "i2", "a2", "u", "alpha", "beta_ab", "t")


def state_of(c):
    """The state and the proposal of a case: what tests.test_gpu_wgibbs.synthetic_state returns."""
    return {k: c[k] for k in STATE_KEYS}


def finish(name, s, **extra):
    """The oracle's result next to the state `s` (the keys of tests.test_gpu_wgibbs.synthetic_state)."""
    c = dict(s, name=name, n_slots=1, slot=0)
    c.update(extra)
    c["w"] = np.ascontiguousarray(c["w"], dtype=F32)
    c["a2"] = np.ascontiguousarray(c["a2"], dtype=np.float64)
    c["u"] = np.ascontiguousarray(c["u"], dtype=F32)
    c["alpha"] = np.ascontiguousarray(c["alpha"], dtype=np.float64)
    c["beta_ab"] = np.ascontiguousarray(c["beta_ab"], dtype=np.float64)
    c["t"] = float(c["t"])
    patterns, pid = np.unique(c["has_components"], axis=0, return_inverse=True)
    c["patterns"], c["pid"] = patterns, np.asarray(pid).reshape(-1)
    c["w_new"], c["a2_old"] = worc.propose_weights(c["w"], c["i1"], c["i2"], c["a2"])
    c["w_out"], c["accept"], c["terms"], _ = worc.step(c["w"], patterns, c["pid"], c["src"], c["na"], c["i1"], c["i2"], c["a2"],
                                                       c["u"], c["alpha"], c["beta_ab"], c["t"])
    c["band"] = worc.device_band(c["terms"], c["t"])
    c["margin"] = worc.log_margin(c["u"], c["terms"]["log_p"])
    c["cls"] = classes(c["terms"]["log_p"])
    fin = c["cls"] == FINITE
    if not (c["margin"][fin] > 2 * c["band"][fin]).all():
        raise Refused(f"{name}: features {np.flatnonzero(fin & ~(c['margin'] > 2 * c['band'])).tolist()} decide within twice the band")
    for v in list(c.values()) + list(c["terms"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- the high-precision reference ------------------------------------------------------------------------------------------
def mp_log_p(c):
    """The contract's log ratio at 50 digits, per feature with a finite oracle log_p (None elsewhere).  The inputs are the
    contract's float32 quantities -- w, w_new, the per-pattern normalised tables, a2_old -- and its float64 coefficients
    alpha - 1, A - 1, B - 1 (exact by definition); every log and log1p is mpmath's, a term whose coefficient is 0 is left
    out, the likelihood term is grouped by (pattern, component) with integer counts, the sum is divided by T."""
    if "_mp" in c:
        return c["_mp"]
    P, C = c["patterns"].shape
    F = c["w"].shape[0]
    told, tnew = worc.normalized_weights(c["w"], c["patterns"]), worc.normalized_weights(c["w_new"], c["patterns"])
    out = [None] * F
    with mpmath.workdps(MP_DIGITS):
        mpf, log, log1p = mpmath.mpf, mpmath.log, mpmath.log1p
        for f in np.flatnonzero(c["cls"] == FINITE):
            seen = ~c["na"][:, f]
            cnt = np.bincount(c["pid"][seen] * C + c["src"][seen, f], minlength=P * C).reshape(P, C)   # (finite: every source >= 0)
            total = mpf(0)
            for p, k in zip(*np.nonzero(cnt)):
                total += int(cnt[p, k]) * (log(mpf(float(tnew[p, f, k]))) - log(mpf(float(told[p, f, k]))))
            for k in range(C):
                coef = float(c["alpha"][f, k] - 1.0)
                if coef != 0.0:
                    total += mpf(coef) * (log(mpf(float(c["w_new"][f, k]))) - log(mpf(float(c["w"][f, k]))))
            a, ao = mpf(float(c["a2"][f])), mpf(float(c["a2_old"][f]))
            ca, cb = float(c["beta_ab"][f, 0] - 1.0), float(c["beta_ab"][f, 1] - 1.0)
            if ca != 0.0:
                total += mpf(ca) * (log(ao) - log(a))
            if cb != 0.0:
                total += mpf(cb) * (log1p(-ao) - log1p(-a))
            out[f] = total / mpf(c["t"])
    c["_mp"] = out
    return out


def distance_to_mp(c, log_p):
    """float64 [F]: |log_p - mp| / band per finite feature (NaN elsewhere); a band of 0 asks for equality (0, or inf)."""
    out = np.full(len(log_p), np.nan)
    with mpmath.workdps(MP_DIGITS):
        for f, m in enumerate(mp_log_p(c)):
            if m is not None:
                d, b = abs(mpmath.mpf(float(log_p[f])) - m), mpmath.mpf(float(c["band"][f]))
                out[f] = float(d / b) if b > 0 else (0.0 if d == 0 else np.inf)
    return out


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def objects_of(rng, n, patterns):
    """has_components bool [n, C]: the rows of `patterns`, each as often as the others (every one occurs for n >= P), shuffled."""
    patterns = np.asarray(patterns, dtype=bool)
    return patterns[rng.permutation(n) % len(patterns)]


def sources_of(rng, hc, allowed, na_rate):
    """(src int16 [N, F], na bool [N, F]): per observation one of the components of the object's pattern that `allowed[f]`
    permits, drawn uniformly; NA where there is none, and at `na_rate` elsewhere."""
    n, f = hc.shape[0], allowed.shape[0]
    score = (rng.random((n, f, hc.shape[1])) + 0.01) * (hc[:, None, :] & allowed[None, :, :])
    src = score.argmax(axis=-1).astype(np.int16)
    na = (score.max(axis=-1) == 0) | (rng.random((n, f)) < na_rate)
    src[na] = -1
    return src, na


def neutralise(w, i1, i2, a2, alpha, beta_ab):
    """What keeps log_p finite next to zeros: alpha = 1 exactly on a component whose weight or proposed weight is 0, A = 1
    exactly where a2 or a2_old is 0, B = 1 exactly where a2 or a2_old is 1 -- coefficient 0 against an infinite log.  Returns
    `allowed` bool [F, C]: the components an observation may have as its source (a weight above 0 on both sides)."""
    w_new, a2_old = worc.propose_weights(w, i1, i2, a2)
    zero = (w == 0) | (w_new == 0)
    alpha[zero] = 1.0
    beta_ab[(a2 == 0) | (a2_old == 0), 0] = 1.0
    beta_ab[(a2 == 1) | (a2_old == 1), 1] = 1.0
    return ~zero & ~np.isnan(w_new)


# ---- A: weight magnitudes and the row sum ---------------------------------------------------------------------------------
SMALL = (0.0, 2.0 ** -149, 2.0 ** -126, 1e-30, 1e-20, 1e-10, 2.0 ** -24)
PLACES = ("i1", "i2", "other", "both")
A_N = 300


def a_pairs(c):
    if c <= 4:
        return list(itertools.permutations(range(c), 2))
    return [(0, c - 1), (c - 1, 0), (2, c - 2)]


def a_rows(c):
    """(value, place) of every overwritten row; two plain rows follow them."""
    return [(v, place) for v in SMALL for place in PLACES if place != "other" or c > 2]


def a_patterns(c, i1, i2):
    ones = np.ones(c, dtype=bool)
    rows = [ones.copy() for _ in range(4)]
    rows[1][i1] = False
    rows[2][i2] = False
    rows[3][[i1, i2]] = False
    other = [k for k in range(c) if k not in (i1, i2)]
    for k in [i1, i2] + other[:1]:
        rows.append(np.arange(c) == k)
    rows = np.unique(np.array(rows), axis=0)
    return rows[rows.any(axis=1)]


def group_a(c, i1, i2):
    rng = np.random.default_rng(1000 + 100 * c + 10 * i1 + i2)
    rows = a_rows(c)
    f = len(rows) + 2
    other = [k for k in range(c) if k not in (i1, i2)]
    w = rng.dirichlet(np.full(c, 2.0), f).astype(F32)
    for r, (v, place) in enumerate(rows):
        at = {"i1": [i1], "i2": [i2], "both": [i1, i2], "other": other[r % len(other):][:1] if other else []}[place]
        w[r, at] = F32(v)
    a2 = rng.uniform(0.3, 0.7, f)
    alpha = rng.choice([0.3, 0.5, 2.5], (f, c))
    beta_ab = 1.0 + rng.random((f, 2)) * 20
    allowed = neutralise(w, i1, i2, a2, alpha, beta_ab)
    hc = objects_of(rng, A_N, a_patterns(c, i1, i2))
    src, na = sources_of(rng, hc, allowed, 0.1)
    s = dict(w=w, has_components=hc, src=src, na=na, i1=i1, i2=i2, a2=a2, u=rng.random(f, dtype=F32), alpha=alpha, beta_ab=beta_ab,
             t=float(rng.choice([1.0, 1.5])))
    want = np.array([NAN if (v, place) == (0.0, "both") else FINITE for v, place in rows] + [FINITE, FINITE])
    return finish(f"A_c{c}_{i1}_{i2}", s, rows=rows, built_for=want)


# ---- B: draws, priors, temperatures and the four classes of log_p ------------------------------------------------------------
B_A2 = (0.0, 1.0, 2.0 ** -1074, 1e-300, 1e-20, 2.0 ** -30, 0.5, 1.0 - 2.0 ** -53)
B_COUNTS = (0.0, 1.0, 1e3, 1e6)
B_ALPHA = (1e-3, 0.3, 2.5, 1e4)
B_T = (1e-3, 1.0, 1.5, 1e3)
B_U = (0.0, 2.0 ** -149, 2.0 ** -126, 1e-10, 0.5, 1.0 - 2.0 ** -24)
B_PLAN = (FINITE, FINITE, PINF, NINF, NAN, FINITE, FINITE, FINITE)          # per feature, cycled
B_F, B_N, B_C = 72, 200, 4


def group_b(k):
    t = B_T[k]
    rng = np.random.default_rng(2000 + k)
    c, f, n = B_C, B_F, B_N
    i1, i2 = ((1, 3), (3, 0), (0, 2), (2, 1))[k]
    o1, o2 = [j for j in range(c) if j not in (i1, i2)]
    built_for = np.array([B_PLAN[j % len(B_PLAN)] for j in range(f)])
    w = rng.dirichlet(np.full(c, 2.0), f).astype(F32)
    a2 = np.array([B_A2[(j // 2 + j) % len(B_A2)] for j in range(f)])
    counts = np.array([[B_COUNTS[j % 4], B_COUNTS[(j // 4 + j // 16) % 4]] for j in range(f)])
    beta_ab = worc.beta_parameters(counts, np.full((f, c), 0.5, dtype=F32), 0, 1, t)
    alpha = np.array([[B_ALPHA[(j + 3 * m) % 4] for m in range(c)] for j in range(f)])
    u = np.array([B_U[j % len(B_U)] for j in range(f)], dtype=F32)
    fin = np.flatnonzero(built_for == FINITE)
    w[fin[::5], o1] = 0.0                                   # a zero weight outside the pair: alpha = 1 exactly below
    # every pattern has i1 (the +inf features need it); half have i2, and the others vary
    pats = np.array([[True, a, b, d] for a in (True, False) for b in (True, False) for d in (True, False)])
    pats = pats[:, np.argsort([i1, i2, o1, o2])]
    hc = objects_of(rng, n, pats)
    kinds = np.zeros(f, dtype=int)
    for cls in (PINF, NINF, NAN):
        idx = np.flatnonzero(built_for == cls)
        kinds[idx] = np.arange(len(idx))
    only = {}                                               # feature -> the one source of its observations
    no_source = []
    for j in range(f):
        v = kinds[j]
        if built_for[j] == PINF:                            # a2 = 0: log a2 and log w_new[i2] are -inf
            a2[j], only[j], u[j] = 0.0, i1, 1.0 - 2.0 ** -24
            alpha[j, i2], beta_ab[j, 0] = ((0.3, 1.0), (1.0, beta_ab[j, 0] + 1.0), (1e-3, beta_ab[j, 0] + 1.0))[v % 3]
        elif built_for[j] == NINF:
            u[j] = 0.0
            if v % 3 == 0:                                  # sources at i2, whose proposed weight is 0: the likelihood term
                a2[j], only[j], alpha[j, i2], beta_ab[j, 0] = 0.0, i2, 1.0, 1.0
            elif v % 3 == 1:                                # a2_old = 0 under A > 1: the proposal term
                w[j, i2], a2[j], alpha[j, i2], beta_ab[j, 0] = 0.0, 0.5, 1.0, beta_ab[j, 0] + 1.0
            else:                                           # a2 = 1: w_new[i1] = 0 under alpha > 1, B = 1 exactly: the prior term
                a2[j], alpha[j, i1], beta_ab[j, 1] = 1.0, 2.5, 1.0
        elif built_for[j] == NAN:
            u[j] = 0.0
            if v % 4 == 0:                                  # w02 = 0: a NaN row and a NaN a2_old
                w[j, [i1, i2]] = 0.0
            elif v % 4 == 1:                                # an observation without a source component
                no_source.append(j)
                a2[j] = 0.5
            elif v % 4 == 2:                                # +inf from the proposal term meets -inf from the prior term
                a2[j], only[j], alpha[j, i2], beta_ab[j, 0] = 0.0, i1, 2.5, beta_ab[j, 0] + 1.0
            else:                                           # a zero weight outside the pair under alpha != 1: -inf - -inf
                w[j, o2], a2[j], alpha[j, o2] = 0.0, 0.5, 0.3
    w_new, a2_old = worc.propose_weights(w, i1, i2, a2)
    zero = (w == 0) | (w_new == 0)
    keep = built_for == FINITE                              # the finite features: coefficient 0 against every infinite log
    alpha[keep[:, None] & zero] = 1.0
    beta_ab[keep & ((a2 == 0) | (a2_old == 0)), 0] = 1.0
    beta_ab[keep & ((a2 == 1) | (a2_old == 1)), 1] = 1.0
    allowed = ~zero & ~np.isnan(w_new)
    for j, comp in only.items():
        allowed[j] = np.arange(c) == comp
    src, na = sources_of(rng, hc, allowed, 0.1)
    for j in no_source:
        row = int(np.flatnonzero(~na[:, j])[0])
        src[row, j] = -1
    s = dict(w=w, has_components=hc, src=src, na=na, i1=i1, i2=i2, a2=a2, u=u, alpha=alpha, beta_ab=beta_ab, t=t)
    return finish(f"B_T{t:g}", s, built_for=built_for)


# ---- C: decisions at close range -----------------------------------------------------------------------------------------------
C_STATES = ((1, 37, 21, 3, None), (3, SWEEP + 1, 17, 4, None), (4, 3 * SWEEP + 5, 50, 4, None), (5, 1300, 33, 8, 40))
C_SIDES = ("below", "above", "two_below")
C_NUDGES = (0.02, -0.02, 0.05, -0.05, 0.1, -0.1, 0.2, -0.2)


def _oracle_log_p(s):
    patterns, pid = np.unique(s["has_components"], axis=0, return_inverse=True)
    terms = worc.step(s["w"], patterns, np.asarray(pid).reshape(-1), s["src"], s["na"], s["i1"], s["i2"], s["a2"], s["u"], s["alpha"],
                      s["beta_ab"], s["t"])[2]
    return terms["log_p"], worc.device_band(terms, s["t"])


def _open(log_p):
    """p32 = float32(exp(log_p)) has float32 neighbours on both sides inside (0, 1) and is normal."""
    with np.errstate(over="ignore", invalid="ignore"):
        p32 = np.exp(log_p).astype(F32)
        return (p32 > F32(2.0 ** -126)) & (np.nextafter(p32, F32(2)) < F32(1))


@functools.lru_cache(maxsize=None)
def c_state(k):
    """The state of C_STATES[k], with a2 moved next to a2_old on the features whose p lies outside (2^-126, 1): that brings
    log_p near 0, and the first nudge that gives p < 1 is kept."""
    seed, n, f, c, n_patterns = C_STATES[k]
    s = synthetic_state(seed, n, f, c, n_patterns)
    a2_old = worc.propose_weights(s["w"], s["i1"], s["i2"], s["a2"])[1].astype(np.float64)
    log_p, _ = _oracle_log_p(s)
    for d in C_NUDGES:
        bad = ~_open(log_p)
        if not bad.any():
            break
        trial = dict(s, a2=np.where(bad, np.clip(a2_old * (1 + d), 1e-6, 1 - 1e-6), s["a2"]))
        trial_log_p, _ = _oracle_log_p(trial)
        better = bad & _open(trial_log_p)
        s["a2"] = np.where(better, trial["a2"], s["a2"])
        log_p = np.where(better, trial_log_p, log_p)
    return s


def group_c(k, side):
    s = dict(c_state(k))
    log_p, band = _oracle_log_p(s)
    is_open = _open(log_p)
    with np.errstate(over="ignore"):
        p32 = np.exp(log_p).astype(F32)
    below, above = np.nextafter(p32, F32(-1)), np.nextafter(p32, F32(2))
    u = {"below": below, "above": above, "two_below": np.nextafter(below, F32(-1))}[side]
    with np.errstate(invalid="ignore"):
        close = is_open & (worc.log_margin(np.where(is_open, u, F32(0.5)), log_p) > 2 * band)
    s["u"] = np.where(close, u, F32(0.5)).astype(F32)
    seed, n, f, c, _ = C_STATES[k]
    return finish(f"C_n{n}_c{c}_{side}", s, close=close, side=side)


# ---- D: shapes and places ------------------------------------------------------------------------------------------------------
D_N = (1, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP - 1, 2 * SWEEP + 1, 8 * SWEEP + 3)
D_F = (1, 15, 16, 17, 33)
D_SPECIAL = ("all_na", "last_object_only", "all_i1", "all_i2")


def _special_features(s):
    """Features 0 to 3 of the table become D_SPECIAL (as far as F reaches)."""
    hc, src, na, i1, i2 = s["has_components"], s["src"], s["na"], s["i1"], s["i2"]
    n, f = src.shape
    last = int(np.flatnonzero(hc[n - 1])[0])
    for j, kind in enumerate(D_SPECIAL[:f]):
        if kind == "all_na":
            na[:, j] = True
        elif kind == "last_object_only":
            na[:, j] = True
            na[n - 1, j], src[n - 1, j] = False, last
        else:
            comp = i1 if kind == "all_i1" else i2
            na[:, j] |= ~hc[:, comp]
            src[:, j] = comp
        src[na[:, j], j] = -1
    return s


def group_d_objects(n):
    f, c = (19, 2) if n == D_N[-1] else (6, 3)
    s = _special_features(synthetic_state(4000 + n, n, f, c))
    return finish(f"D_n{n}", s, special=D_SPECIAL[:f])


D_TILE_SEEDS = {7: 4107, 8: 4115}         # (at C = 8 the 64 patterns that synthetic_state keeps are without component 0: a pair without it)


def group_d_tile(c):
    s = _special_features(synthetic_state(D_TILE_SEEDS[c], 900, 17, c, 64))
    return finish(f"D_p64_c{c}", s, special=D_SPECIAL)


def group_d_features(f):
    return finish(f"D_f{f}", synthetic_state(4200 + f, 150, f, 3))


def group_d_slot():
    return finish("D_slot2_of_3", _special_features(synthetic_state(4300, 301, 18, 3)), n_slots=3, slot=2, special=D_SPECIAL)


# ---- the table of cases ----------------------------------------------------------------------------------------------------
CASES = {}
for _c in range(2, 9):
    for _i1, _i2 in a_pairs(_c):
        CASES[f"A_c{_c}_{_i1}_{_i2}"] = functools.partial(group_a, _c, _i1, _i2)
for _k, _t in enumerate(B_T):
    CASES[f"B_T{_t:g}"] = functools.partial(group_b, _k)
for _k, (_seed, _n, _f, _c, _p) in enumerate(C_STATES):
    for _side in C_SIDES:
        CASES[f"C_n{_n}_c{_c}_{_side}"] = functools.partial(group_c, _k, _side)
for _n in D_N:
    CASES[f"D_n{_n}"] = functools.partial(group_d_objects, _n)
for _c in (7, 8):
    CASES[f"D_p64_c{_c}"] = functools.partial(group_d_tile, _c)
for _f in D_F:
    CASES[f"D_f{_f}"] = functools.partial(group_d_features, _f)
CASES["D_slot2_of_3"] = group_d_slot

PLACE_CASE = "A_c8_0_7"                   # two feature tiles: a rotation by 5 moves features across the tile edge


def group(letter):
    return [name for name in CASES if name.startswith(letter + "_")]


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert c["name"] == name
    return c


def replaced(c, order):
    """The state and proposal of case `c` with its features in `order`: feature j of the result is feature order[j] of c."""
    order = np.asarray(order)
    return dict(state_of(c), n_slots=c["n_slots"], slot=c["slot"], w=c["w"][order], src=c["src"][:, order], na=c["na"][:, order], a2=c["a2"][order], u=c["u"][order],
                alpha=c["alpha"][order], beta_ab=c["beta_ab"][order])
