"""The range cases of the per-pattern normalised weights (k_weight_patterns / k_scatter_weight_patterns / k_expand_weights and
the row form k_normalize_weight_rows, sbayes_amd/csrc/sbe_kernels.hip.h), of the per-object source prior (k_source_prior and the
object blocks of k_collapsed_source_prior, sbe_kernels_sampling.hip.h) and of k_source_lh_by_feature
(sbe_kernels_operators.hip.h), shared by tests/test_srcprior_range_cpu.py (which proves under the NumPy oracle and mpmath alone
that every case is what it claims) and tests/test_gpu_srcprior_range.py (device against oracle and 50-digit values).  DESIGN.md
section 4.3c.  Four groups:

    W  normalisation: C from 1 to 8; 0, float32 denormals and small normals at every place of the row beside ordinary weights;
       every has_components pattern at C <= 4 (the empty one: a masked sum of 0), as many patterns as the engine holds
       (min(2^C, 64)) above; all-denormal rows; rows of wide dynamic range at C = 8 whose chained float32 sum is not NumPy's;
       inf and NaN under a cleared and under a set bit; F and F*C at every remainder mod 4; P*F around the 256-thread block;
       for the row form 1, 7, 8, 9, 17 and 300 rows, the largest table the row kernel stages in LDS and the smallest beyond it.
    P  source prior: F in (1, 63, 64, 65, 129) x N in (1, 15, 16, 17, 33), C in (1, 3, 8); objects all NA, of one observation,
       with a 0xFF source on an observed cell, with sources whose normalised weight is 0, 1, denormal or NaN, with every source
       at the last component; the logf grid (one observation per object, normalised weights in every binade from 2^-149 to 1);
       the last of three slots.
    L  source likelihood by feature: N in (1, 63, 64, 65, 511, 512, 513, 1025), F in (1, 15, 16, 17, 33), the same value
       classes by feature, one feature NA throughout, one with a single -inf; the grid state.
    E  the accumulation, exactly: finite states in which every object (or every feature) has one observation, so that one of
       the two kernels returns the device's float32 logs one by one and the other's sum can be held to their float64 sum
       rounded once (`exactly_rounded`); up to 1025 objects of a feature, up to 129 features of an object.

A W case is a dict of the weights `w` [F, C], the rows `hc` [N, C], the oracle's `want` [N, F, C] (orc.normalize_weights) and
`wpat`, `pid` (orc.weight_patterns), and -- `mp_normalized` -- the 50-digit quotients and their bands per (pattern, f, c).  A
P / L case is a dict of `w`, `hc`, `src` (component per observation, -1: none), `na`, the oracle's normalised weights `wn`,
`prior` [N] (orc.source_prior_per_object) and `by_feature` [F] (orc.source_lh_by_feature), and -- `mp_sums` -- the 50-digit
sums of the logs of the float32 normalised weights AS THE ORACLE ROUNDS THEM, with what the band needs.  `case(name)` computes a
case once; its arrays are read-only."""
from __future__ import annotations

import functools
import itertools
import math

import mpmath
import numpy as np

from oracle import sbayes_oracle as orc
from tests._wgibbs_cases import source_array
from tests._wgibbs_range_cases import FINITE, NAN, NINF, PINF, SMALL, class_counts, classes, objects_of, sources_of  # noqa: F401

MP_DIGITS = 50
F32 = np.float32
U = 2.0 ** -24                            # float32 unit roundoff
TINY = 2.0 ** -149                        # the smallest float32 denormal
MIN_NORMAL = 2.0 ** -126
MAX_PATTERNS = 64                         # the engine holds min(2^C, 64) has_components patterns per slot (sbe_mixture_plan.h)
ROW_STATIC_LDS = 8 * 4                    # k_normalize_weight_rows' static part: the pattern bits of its 8 rows
ROW_LDS_BUDGET = (64 << 10) - ROW_STATIC_LDS   # sbe_normalize_weights: weights of F * C * 4 bytes beyond it are read in place
ROW_MAPPED_LIMIT = 256                    # ... and up to this many rows read them out of the mapped ring (test_gpu_host_paths.py)


def capacity(c):
    return min(1 << c, MAX_PATTERNS)


def ulp32(x):
    """The float32 spacing at |x| (2^-149 below 2^-126)."""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), MIN_NORMAL)
    return np.exp2(np.floor(np.log2(x)) - 23)


def bits_equal(a, b):
    """Bit for bit, any NaN meeting any NaN (the host's and the device's default NaN differ in the sign bit)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    kind = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(kind)[~na], b.view(kind)[~nb]))


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- W: the oracle and the 50-digit quotients ------------------------------------------------------------------------------------
def masked_rows(w, patterns):
    """float32 [P, F, C]: NumPy's bool * float32 -- 0 * w under a cleared bit, so a NaN or inf stays in the sum."""
    with np.errstate(invalid="ignore"):
        return np.asarray(patterns)[:, None, :] * np.asarray(w, dtype=F32)[None, :, :]


def chained_normalize(w, patterns):
    """float32 [P, F, C]: the quotients under a left-to-right float32 chain instead of NumPy's sum."""
    m = masked_rows(w, patterns)
    total = np.zeros(m.shape[:2], dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(m.shape[2]):
            total = total + m[..., k]
        return m / total[..., None]


def finish_w(name, w, hc, slot_form=True, n_slots=1, slot=0, **extra):
    w = np.ascontiguousarray(w, dtype=F32)
    hc = np.ascontiguousarray(hc, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        want = orc.normalize_weights(w, hc)
        wpat, pid = orc.weight_patterns(w, hc)
    patterns = np.unique(hc, axis=0)
    assert want.dtype == F32 and wpat.shape == (len(patterns),) + w.shape
    c = dict(name=name, w=w, hc=hc, want=want, wpat=wpat, pid=pid, patterns=patterns, slot_form=slot_form, n_slots=n_slots, slot=slot)
    c.update(extra)
    assert not slot_form or len(patterns) <= capacity(w.shape[1]), name
    return _freeze(c)


def mp_normalized(c):
    """(value, band) per (pattern, f, c): object arrays [P, F, C] of mpf, None where the arithmetic gives NaN or an infinity.
    From the float32 weights as stored: m_c = w_c under a set bit, 0 * w_c under a cleared one, S = sum m (exact), value =
    m_c / S.  Band (module docstring of tests/test_gpu_srcprior_range.py): the float32 sum of C terms is S (1 + d) with
    |d| <= g = (C - 1) u / (1 - (C - 1) u) -- a float32 addition whose result is denormal is exact, so the sum carries no absolute
    floor -- and the division rounds once, u relative or 2^-149 where the quotient is denormal:
        band = value * (g + u (1 + g)) + 2^-149.
    A masked inf makes S infinite: the finite entries of such a row are exactly 0 (band 0)."""
    if "_mp" in c:
        return c["_mp"]
    w, patterns = c["w"], c["patterns"]
    m32 = masked_rows(w, patterns)
    P, F, C = m32.shape
    value, band = np.full((P, F, C), None, dtype=object), np.full((P, F, C), None, dtype=object)
    with mpmath.workdps(MP_DIGITS):
        mpf = mpmath.mpf
        u, floor = mpf(2) ** -24, mpf(2) ** -149
        g = (C - 1) * u / (1 - (C - 1) * u)
        rel = g + u * (1 + g)
        for p in range(P):
            for f in range(F):
                row = m32[p, f]
                if np.isnan(row).any():
                    continue
                assert (row >= 0).all()
                if np.isinf(row).any():
                    for k in np.flatnonzero(np.isfinite(row)):
                        value[p, f, k], band[p, f, k] = mpf(0), mpf(0)
                    continue
                m = [mpf(float(v)) for v in row]
                total = mpmath.fsum(m)
                if total == 0:
                    continue
                for k in range(C):
                    v = m[k] / total
                    value[p, f, k], band[p, f, k] = v, v * rel + floor
    c["_mp"] = (value, band)
    return c["_mp"]


def w_distance(c, got_pat):
    """float64 [P, F, C]: |got - value| / band where the 50-digit value exists (NaN elsewhere); a band of 0 asks for equality."""
    value, band = mp_normalized(c)
    out = np.full(value.shape, np.nan)
    with mpmath.workdps(MP_DIGITS):
        for idx in zip(*np.nonzero(value != None)):   # noqa: E711  (object array: elementwise)
            x = float(got_pat[idx])
            if not math.isfinite(x):
                out[idx] = np.inf
                continue
            d, b = abs(mpmath.mpf(x) - value[idx]), band[idx]
            out[idx] = float(d / b) if b > 0 else (0.0 if d == 0 else np.inf)
    return out


def w_row_distance(c, got):
    """Worst |got - value| / band over an [N, F, C] result: per row the pattern's distances, computed once per distinct row."""
    ref = w_distance(c, c["wpat"])
    worst, seen = 0.0, {}
    for n in range(got.shape[0]):
        p = int(c["pid"][n])
        if bits_equal(got[n], c["wpat"][p]):
            d = ref[p]
        else:
            key = (p, got[n].tobytes())
            if key not in seen:
                pat = np.array(c["wpat"])
                pat[p] = got[n]
                seen[key] = w_distance(c, pat)[p]
            d = seen[key]
        fin = ~np.isnan(d)
        worst = max(worst, float(np.max(d[fin], initial=0.0)))
    return worst


# ---- W: the cases ----------------------------------------------------------------------------------------------------------------
def all_patterns(c):
    return np.array(list(itertools.product((False, True), repeat=c)), dtype=bool)


def w_patterns(rng, c):
    """Every pattern at C <= 4 (and wherever the engine holds them all); above, as many as it holds: the empty one, the full
    one, every single component, the rest drawn."""
    every = all_patterns(c)
    if len(every) <= capacity(c):
        return every
    key = lambda row: int("".join("1" if b else "0" for b in row), 2)   # noqa: E731
    must = [np.zeros(c, dtype=bool), np.ones(c, dtype=bool)] + [np.arange(c) == k for k in range(c)]
    have = {key(r) for r in must}
    rest = [r for r in every[rng.permutation(len(every))] if key(r) not in have][:capacity(c) - len(must)]
    return np.array(must + rest)


def plain_rows(rng, n, c):
    return rng.dirichlet(np.full(c, 2.0), n).astype(F32)


def group_w_small(c):
    """The small values at every place of the row, two all-denormal rows, two plain rows; every pattern the engine holds."""
    rng = np.random.default_rng(5000 + c)
    rows = [(v, k) for v in SMALL for k in range(c)]
    w = plain_rows(rng, len(rows) + 4, c)
    for r, (v, k) in enumerate(rows):
        w[r, k] = F32(v)
    w[len(rows)] = F32(TINY)                                                  # C = 3: 2^-149 / (3 * 2^-149) = 0.33333334
    w[len(rows) + 1] = (rng.integers(1, 1000, c) * TINY).astype(F32)
    pats = w_patterns(rng, c)
    hc = np.concatenate([pats, pats[rng.integers(0, len(pats), 3)]])[rng.permutation(len(pats) + 3)]
    return finish_w(f"W_small_c{c}", w, hc, rows=rows, all_denormal=(len(rows), len(rows) + 1))


WIDE_ROWS, WIDE_POOL = 96, 400


def group_w_wide():
    """C = 8, weights exp(6 N(0, 1)): rows whose quotients under the full pattern differ between a chained float32 sum and
    NumPy's tree ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), and eight rows for which they do not."""
    rng = np.random.default_rng(5100)
    pool = np.exp(6.0 * rng.standard_normal((WIDE_POOL, 8))).astype(F32)
    full = np.ones((1, 8), dtype=bool)
    differ = (chained_normalize(pool, full)[0] != orc.normalize_weights(pool, full)[0]).any(axis=1)
    w = np.concatenate([pool[differ][:WIDE_ROWS], pool[~differ][:8]])
    pats = np.array([np.ones(8, dtype=bool), np.arange(8) < 7, np.arange(8) % 2 == 0, np.arange(8) >= 3])
    return finish_w("W_wide_c8", w, pats[[0, 1, 2, 3, 0]], n_differ=min(int(differ.sum()), WIDE_ROWS))


def group_w_nonfinite(c):
    """inf and NaN at every place of an ordinary row; patterns that clear and that set the place's bit."""
    rng = np.random.default_rng(5200 + c)
    rows = [(v, k) for v in (np.inf, np.nan) for k in range(c)]
    w = plain_rows(rng, len(rows) + 1, c)
    for r, (v, k) in enumerate(rows):
        w[r, k] = F32(v)
    if c <= 4:
        pats = all_patterns(c)
    else:
        pats = np.array([np.ones(c, dtype=bool)] + [np.arange(c) != k for k in range(c)] + [np.arange(c) == k for k in range(c)])
    return finish_w(f"W_nonfinite_c{c}", w, pats, rows=rows)


W_SHAPES = ((1, 1), (1, 2), (1, 3), (15, 3), (16, 5), (17, 2), (17, 3), (33, 5), (33, 8),          # F, C: F * C mod 4 = 1 2 3 1 0 2 3 1 0
            (16, 4))                                                                              # 16 patterns x 16 features: P * F = 256
W_BLOCK_F = (255, 256, 257)                                                                       # one pattern, C = 1: P * F around a block


def _sprinkle(rng, w):
    """Small values at a tenth of the places (not the last component, so that the full pattern's sum stays ordinary)."""
    if w.shape[1] > 1:
        at = rng.random(w[:, :-1].shape) < 0.1
        w[:, :-1][at] = rng.choice(np.array(SMALL, dtype=F32), int(at.sum()))
    return w


def group_w_shape(f, c):
    rng = np.random.default_rng(5300 + 10 * f + c)
    w = _sprinkle(rng, plain_rows(rng, f, c))
    pats = w_patterns(rng, c)
    return finish_w(f"W_f{f}_c{c}", w, pats[rng.permutation(len(pats))])


def group_w_block(f):
    rng = np.random.default_rng(5400 + f)
    w = rng.random((f, 1)).astype(F32)
    w[::7, 0] = np.array(SMALL, dtype=F32)[np.arange(len(w[::7])) % len(SMALL)]
    return finish_w(f"W_f{f}_c1", w, np.ones((1, 1), dtype=bool))


W_ROW_COUNTS = (1, 7, 8, 9, 17, 300)      # 8 rows per block; 300 > ROW_MAPPED_LIMIT: the weights go up by copy


def group_w_rows(n):
    """The row form alone (any number of rows, any patterns): F * C = 51 leaves a float4 tail of 3."""
    rng = np.random.default_rng(5500 + n)
    w = _sprinkle(rng, plain_rows(rng, 17, 3))
    pats = all_patterns(3)
    return finish_w(f"W_rows{n}", w, pats[rng.integers(0, len(pats), n)], slot_form=False)


BIG_C = 8
BIG_F = ROW_LDS_BUDGET // (4 * BIG_C) + 1  # the smallest F whose table passes the budget at C = 8


def group_w_big(f=BIG_F, name="W_big_table"):
    """The row form with a table beyond the LDS budget (stage_weights == 0) -- and, at F - 1, the largest table that is staged:
    nine rows of two patterns, the small values at the table's end and two wide rows."""
    rng = np.random.default_rng(5600 + f)
    w = plain_rows(rng, f, BIG_C)
    for r, v in enumerate(SMALL):
        w[f - 1 - r, r % BIG_C] = F32(v)
    w[:2] = np.exp(6.0 * rng.standard_normal((2, BIG_C))).astype(F32)
    pats = np.array([np.ones(BIG_C, dtype=bool), np.arange(BIG_C) % 3 != 1])
    return finish_w(name, w, pats[[0, 1, 1, 0, 1, 0, 0, 1, 1]], slot_form=False)


def group_w_slot():
    rng = np.random.default_rng(5700)
    w = _sprinkle(rng, plain_rows(rng, 21, 3))
    return finish_w("W_slot2_of_3", w, all_patterns(3)[rng.permutation(8)], n_slots=3, slot=2)


# ---- P and L: the oracle and the 50-digit sums -----------------------------------------------------------------------------------
def finish_s(name, w, hc, src, na, n_slots=1, slot=0, **extra):
    w = np.ascontiguousarray(w, dtype=F32)
    hc = np.ascontiguousarray(hc, dtype=bool)
    src = np.ascontiguousarray(src, dtype=np.int16)
    na = np.ascontiguousarray(na, dtype=bool)
    C = w.shape[1]
    assert len(np.unique(hc, axis=0)) <= capacity(C), name
    source = source_array(src, C)
    with np.errstate(invalid="ignore", divide="ignore"):
        wn = orc.normalize_weights(w, hc)
        prior = orc.source_prior_per_object(wn, source, na)
        by_feature = orc.source_lh_by_feature(source, wn, na)
        # the weight the device selects: the source component's, 0 where the observation has none
        picked = np.where(src >= 0, np.take_along_axis(wn, np.maximum(src, 0)[..., None].astype(np.int64), axis=2)[..., 0], F32(0))
    assert prior.dtype == np.float64 and by_feature.dtype == F32 and picked.dtype == F32
    c = dict(name=name, w=w, hc=hc, src=src, na=na, wn=wn, picked=picked, prior=prior, by_feature=by_feature, n_slots=n_slots, slot=slot)
    c.update(extra)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def _mp_log_bits(bits):
    with mpmath.workdps(MP_DIGITS):
        return mpmath.log(mpmath.mpf(float(np.uint32(bits).view(F32))))


def mp_log(v):
    """The 50-digit log of one positive finite float32."""
    return _mp_log_bits(int(np.asarray(v, dtype=F32).view(np.uint32)))


def mp_sums(c, axis):
    """The 50-digit sums of the logs of the float32 weights the device selects, over the features of an object (axis 1:
    the source prior) or the objects of a feature (axis 0: source_lh_by_feature), NA observations left out.  Per sum a dict:
    cls (FINITE, NAN, NINF), exact (mpf, FINITE only), n (terms), sum_ulp = sum ulp32(|log w|), sum_abs = sum |log w|."""
    key = f"_mp{axis}"
    if key in c:
        return c[key]
    picked, seen = c["picked"], ~c["na"]
    if axis == 0:
        picked, seen = picked.T, seen.T
    out = []
    with mpmath.workdps(MP_DIGITS):
        for row, ok in zip(picked, seen):
            vals = row[ok]
            if np.isnan(vals).any():
                out.append(dict(cls=NAN, n=len(vals)))
            elif (vals == 0).any():
                out.append(dict(cls=NINF, n=len(vals)))
            else:
                assert np.isfinite(vals).all()
                logs = [mp_log(v) for v in vals]
                floats = np.array([float(t) for t in logs], dtype=np.float64)
                out.append(dict(cls=FINITE, n=len(vals), exact=mpmath.fsum(logs), sum_ulp=float(np.sum(ulp32(floats)[floats != 0])),
                                sum_abs=float(np.sum(np.abs(floats)))))
    c[key] = out
    return out


def sum_band(s, l_max, adds):
    """|out - exact| <= sum L_max ulp32(|log w|) + 1/2 ulp32(|exact|) + adds * 2^-53 * sum |log w|: every float32 log within
    L_max ulp, `adds` float64 additions on the way of a term, one rounding to float32 (a sum of exactly 0: no term errs)."""
    exact = float(s["exact"])
    return l_max * s["sum_ulp"] + (0.5 * float(ulp32(exact)) if exact != 0 else 0.0) + adds * 2.0 ** -53 * s["sum_abs"]


def s_distance(c, axis, got, l_max, extra=None):
    """float64: |got - exact| / band per finite sum (NaN elsewhere); `extra` (per sum) widens the band (the oracle's own
    float32 accumulation, tests/test_srcprior_range_cpu.py)."""
    sums = mp_sums(c, axis)
    out = np.full(len(sums), np.nan)
    adds = c["w"].shape[0] if axis == 1 else c["na"].shape[0]
    with mpmath.workdps(MP_DIGITS):
        for i, s in enumerate(sums):
            if s["cls"] != FINITE:
                continue
            x = float(got[i])
            if not math.isfinite(x):
                out[i] = np.inf
                continue
            d = abs(mpmath.mpf(x) - s["exact"])
            b = sum_band(s, l_max, adds) + (0.0 if extra is None else float(extra[i]))
            out[i] = float(d / mpmath.mpf(b)) if b > 0 else (0.0 if d == 0 else np.inf)
    return out


def sum_classes(c, axis):
    return np.array([s["cls"] for s in mp_sums(c, axis)])


# ---- the logf grid ---------------------------------------------------------------------------------------------------------------
GRID_MANTISSAS = (1.0, 1.0 + 2.0 ** -23, 1.1802, 1.5, 1.7320508, 2.0 - 2.0 ** -22)


def grid_weights():
    """float32 [G, 2] rows (x, y) and bool [G, 2] patterns whose first normalised weight is the grid: below 2^-25 the row
    (x, 1) under the full pattern gives x / fl(1 + x) = x exactly -- every denormal and small binade, 2^-126 and its predecessor
    --, above it (x, 1 - x) gives a value next to x, (1 - 2^-24, 2^-24) the predecessor of 1, and component 0 alone gives 1.
    From 2^-24 on every x comes a second time as (1 - x, x): weights next to 1, whose logs -x (1 + x / 2 + ...) fill the binades of
    the RESULT between 2^-24 and 1 -- where a float32 log is hardest (NumPy's worst over the grid lies there, at w = 0.78; without
    these rows the grid finds 0.75 ulp for it, with them 2.57)."""
    rows, pats = [], []
    for e in range(-149, 0):
        for m in GRID_MANTISSAS:
            x = F32(m * 2.0 ** e)
            if not 0 < x < 1:
                continue
            rows.append((x, F32(1)) if e < -25 else (x, F32(1) - x))
            pats.append((True, True))
            if e >= -24 and m < 2.0 - 2.0 ** -22:                             # ... and the binades of the LOG next to 0: w = 1 - x,
                rows.append((F32(1) - x, x))                                  # log w = -x (1 + x / 2 + ...), the sum exactly 1
                pats.append((True, True))
    rows += [(F32(MIN_NORMAL), F32(1)), (np.nextafter(F32(MIN_NORMAL), F32(0)), F32(1)), (F32(TINY), F32(1)), (F32(1 - U), F32(U)), (F32(0.7), F32(0.3))]
    pats += [(True, True)] * 4 + [(True, False)]
    rows, keep = np.unique(np.array(rows, dtype=F32), axis=0, return_index=True)
    return rows, np.array(pats, dtype=bool)[keep]


def group_grid():
    """Object n observes feature n alone, source component 0: its prior is float(logf(w_n)), and so is feature n's sum."""
    w, hc = grid_weights()
    g = len(w)
    na = ~np.eye(g, dtype=bool)
    src = np.where(na, -1, 0).astype(np.int16)
    return finish_s("P_grid", w, hc, src, na)


def grid_values(c):
    """float32 [G]: the normalised weight of the one observation of every object, as the oracle rounds it."""
    return np.ascontiguousarray(np.diagonal(c["picked"]))


@functools.lru_cache(maxsize=None)
def l_ref():
    """(L_ref, the weight where it is reached): the worst |float32 NumPy log(w) - log w| over the grid in float32 ulps of the exact
    value -- the reference's own accuracy."""
    v = grid_values(case("P_grid"))
    with np.errstate(divide="ignore"):
        got = np.log(v)
    assert got.dtype == F32
    return log_ulps(v, got)


def log_ulps(v, got):
    """(worst, weight): the largest |got - log v| in float32 ulps of the exact log over the float32 weights `v` (log 1 = 0: equality)."""
    worst, at = 0.0, None
    with mpmath.workdps(MP_DIGITS):
        for x, y in zip(v, got):
            t = mp_log(x)
            if t == 0:
                d = 0.0 if y == 0 else np.inf
            else:
                d = float(abs(mpmath.mpf(float(y)) - t) / mpmath.mpf(float(ulp32(float(t)))))
            if d > worst:
                worst, at = d, float(x)
    return worst, at


L_CAP = 2                                 # the allowance expected of a float32 log; the device needs no more


def l_oracle():
    """ceil(max(1, L_ref)): what the reference's own float32 log needs, rounded up to a whole ulp (3 with NumPy 2.2.6 on the grid
    as extended by the 1 - x rows; 1 without them)."""
    return int(math.ceil(max(1.0, l_ref()[0])))


def l_max():
    """The device's float32 log may be as inexact as the reference's but no worse (the two libraries round differently) --
    and, where the reference needs more than L_CAP ulp, no worse than that."""
    return min(l_oracle(), L_CAP)


# ---- P and L: states with every value class ------------------------------------------------------------------------------------------
KINDS = ("plain", "all_na", "single", "no_source", "zero", "one", "denormal", "nan", "last")
FEATURE_KINDS = ("plain", "plain", "zero", "plain", "denormal", "plain", "nan", "plain")          # by f % 8, from f = 1 on


def s_patterns(rng, c):
    pats = all_patterns(c)[1:]                                                # (not the empty one: its rows are NaN throughout)
    if len(pats) > 12:                                                        # (the kinds below add patterns: 64 hold them all)
        pats = np.concatenate([pats[-1:], pats[rng.permutation(len(pats) - 1)[:11]]])
    return pats


def value_state(seed, n, f, c, first_kind=0, na_rate=0.15):
    """Weights whose features are plain, hold an exact 0 or a relative 1e-42 at component 0, or are 0 throughout (NaN under every
    pattern); objects of KINDS in turn, from `first_kind` on.  Plain observations have a source of positive normalised weight."""
    rng = np.random.default_rng(seed)
    w = plain_rows(rng, f, c)
    fk = np.array(["plain"] + [FEATURE_KINDS[j % 8] for j in range(1, f)])
    w[fk == "zero", 0] = 0.0
    w[fk == "denormal", 0] = F32(1e-42)
    w[fk == "nan"] = 0.0
    if c == 1:                                                                # one component: a weight is 1 or, at 0 / 0, NaN
        w[fk == "denormal", 0] = F32(TINY)
    hc = objects_of(rng, n, s_patterns(rng, c))
    allowed = w > 0                                                           # (none in a feature of zeros: NA for plain objects)
    if c > 1:
        allowed[(fk == "zero") | (fk == "denormal"), 0] = False
    src, na = sources_of(rng, hc, allowed, na_rate)
    kinds = np.array([KINDS[(first_kind + j) % len(KINDS)] for j in range(n)])
    special = {k: np.flatnonzero(fk == k) for k in ("zero", "denormal", "nan")}
    for j, kind in enumerate(kinds):
        seen = np.flatnonzero(~na[j])
        if kind == "all_na":
            na[j] = True
        elif kind == "single":
            keep = seen[:1] if len(seen) else []
            na[j] = True
            na[j, keep] = False
        elif kind == "no_source":                                             # an observed cell without a source component: 0xFF
            at = seen[0] if len(seen) else 0
            na[j, at], src[j, at] = False, -1
        elif kind in ("zero", "denormal") and c > 1:
            hc[j, 0] = hc[j, c - 1] = True
            at = special[kind]
            na[j, at], src[j, at] = False, 0
        elif kind == "nan":
            at = special["nan"][:1]
            na[j, at], src[j, at] = False, int(np.flatnonzero(hc[j])[0])
        elif kind == "one":                                                   # one component present: every weight 1 (or 0 / 0)
            k = int(rng.integers(0, c))
            hc[j] = np.arange(c) == k
            na[j] = rng.random(f) < na_rate
            na[j, w[:, k] == 0] = True
            src[j] = k
        elif kind == "last":
            hc[j, c - 1] = True
            na[j] = (rng.random(f) < na_rate) | (w[:, c - 1] == 0)
            src[j] = c - 1
        src[j, na[j]] = -1
    return w, hc, src, na, kinds, fk


P_F = (1, 63, 64, 65, 129)
P_N = (1, 15, 16, 17, 33)
P_C = (1, 3, 8)


def p_shapes():
    """Every F with every N; C and the kind of the first object in turn."""
    return [(f, n, P_C[(i + j) % 3], (i + 2 * j) % len(KINDS)) for i, f in enumerate(P_F) for j, n in enumerate(P_N)]


def group_p(f, n, c, first_kind):
    w, hc, src, na, kinds, fk = value_state(6000 + 1000 * c + 10 * f + n, n, f, c, first_kind)
    return finish_s(f"P_f{f}_n{n}_c{c}", w, hc, src, na, kinds=kinds, feature_kinds=fk)


def group_p_slot():
    w, hc, src, na, kinds, fk = value_state(6900, 19, 70, 3)
    return finish_s("P_slot2_of_3", w, hc, src, na, n_slots=3, slot=2, kinds=kinds, feature_kinds=fk)


L_N = (1, 63, 64, 65, 511, 512, 513, 1025)
L_F = (1, 15, 16, 17, 33)


def l_shapes():
    """Every N with one F in turn, and every F at N = 513 (one object in the second pass) and at N = 1025."""
    shapes = [(n, L_F[i % 5], P_C[i % 3]) for i, n in enumerate(L_N)]
    shapes += [(n, f, P_C[(i + 1) % 3]) for n in (513, 1025) for i, f in enumerate(L_F) if (n, f) not in {s[:2] for s in shapes}]
    return shapes


def group_l(n, f, c):
    """value_state's objects, then by feature: feature 1 NA throughout, feature 2 with one -inf (an exact 0 at one source)."""
    w, hc, src, na, kinds, fk = value_state(7000 + 100 * f + n + 7 * c, n, f, c, first_kind=n % len(KINDS))
    planned = {}
    if f == 1:                                                                # (the one feature keeps a finite sum: no 0xFF source)
        na[(src[:, 0] < 0), 0] = True
    if f > 1:
        na[:, 1], src[:, 1] = True, -1
        planned["all_na"] = 1
    if f > 2 and c > 1 and n >= 15:                                           # (feature 2 holds an exact 0 at component 0)
        assert fk[2] == "zero"
        back = src[:, 2] <= 0                                                 # what the "zero" and "no_source" objects observe there: NA again
        na[back, 2], src[back, 2] = True, -1
        j = int(np.flatnonzero(hc[:, 0])[-1])
        na[j, 2], src[j, 2] = False, 0
        planned["single_ninf"] = 2
    return finish_s(f"L_n{n}_f{f}_c{c}", w, hc, src, na, kinds=kinds, feature_kinds=fk, planned=planned)


# ---- E: the accumulation, exactly -----------------------------------------------------------------------------------------------
E_SHAPES = (("feature", 1025, 1, 3), ("feature", 1025, 2, 8), ("feature", 513, 3, 3), ("feature", 512, 1, 8), ("feature", 1025, 4, 3),
            ("feature", 1025, 16, 8),
            ("object", 1, 129, 3), ("object", 2, 129, 8), ("object", 3, 129, 3), ("object", 1, 65, 8), ("object", 5, 129, 3),
            ("object", 8, 129, 8), ("object", 16, 129, 3))


def group_e(by, n, f, c):
    """Finite states in which one of the two kernels returns the device's float32 logs ONE BY ONE while the other adds them.
    by = "feature": object j observes feature j % F alone, so source_prior[j] is float(logf(w)) and source_lh_by_feature[f]
    adds the logs of the objects j = f mod F (every tenth object is NA throughout: 0).  by = "object": feature j is observed by
    object j % N alone, so source_lh_by_feature[j] is the log and source_prior[n] adds those of the features j = n mod N."""
    rng = np.random.default_rng(8000 + 10 * n + f + c)
    w = plain_rows(rng, f, c)
    hc = objects_of(rng, n, s_patterns(rng, c))
    src, na = sources_of(rng, hc, w > 0, 0.0)
    nn, ff = np.meshgrid(np.arange(n), np.arange(f), indexing="ij")
    if by == "feature":
        na |= (ff != nn % f) | (nn % 10 == 9)
    else:
        na |= nn != ff % n
    src[na] = -1
    return finish_s(f"E_{by}_n{n}_f{f}_c{c}", w, hc, src, na, by=by)


def exactly_rounded(got, terms):
    """(ok, exact): whether the float32 `got` is the float64-accumulated sum of the float32 `terms` rounded once: float32 of the
    exact sum (math.fsum), or its neighbour where the exact sum lies within the float64 adds' own error, len * 2^-53 * sum |t|,
    of the midpoint between the two."""
    terms = np.asarray(terms, dtype=np.float64)
    exact = math.fsum(terms.tolist())
    want, got = F32(exact), F32(got)
    if got == want:
        return True, exact
    slack = 2.0 * len(terms) * 2.0 ** -53 * float(np.abs(terms).sum())
    neighbour = got in (np.nextafter(want, F32(np.inf)), np.nextafter(want, F32(-np.inf)))
    return bool(neighbour and abs(abs(exact - float(got)) - abs(exact - float(want))) <= slack), exact


def float32_by_feature(terms):
    """What k_source_lh_by_feature would return for one feature with a float32 accumulator: `terms` [N] (0 for NA), object j on
    lane j % 64, a lane's objects in order, the fixed tree over the 64 lanes."""
    lanes = np.zeros(64, dtype=F32)
    for j, t in enumerate(np.asarray(terms, dtype=F32)):
        lanes[j % 64] = lanes[j % 64] + t
    half = 32
    while half:
        lanes[:half] = lanes[:half] + lanes[half:2 * half]
        half //= 2
    return lanes[0]


float32_by_object = float32_by_feature    # source_prior_block: feature j on lane j % 64, the wave's shuffle tree -- the same shape


# ---- the table of cases ----------------------------------------------------------------------------------------------------------
CASES = {}
for _c in range(1, 9):
    CASES[f"W_small_c{_c}"] = functools.partial(group_w_small, _c)
CASES["W_wide_c8"] = group_w_wide
for _c in (4, 8):
    CASES[f"W_nonfinite_c{_c}"] = functools.partial(group_w_nonfinite, _c)
for _f, _c in W_SHAPES:
    CASES[f"W_f{_f}_c{_c}"] = functools.partial(group_w_shape, _f, _c)
for _f in W_BLOCK_F:
    CASES[f"W_f{_f}_c1"] = functools.partial(group_w_block, _f)
for _n in W_ROW_COUNTS:
    CASES[f"W_rows{_n}"] = functools.partial(group_w_rows, _n)
CASES["W_big_table"] = group_w_big
CASES["W_full_lds"] = functools.partial(group_w_big, BIG_F - 1, "W_full_lds")
CASES["W_slot2_of_3"] = group_w_slot
for _f, _n, _c, _k in p_shapes():
    CASES[f"P_f{_f}_n{_n}_c{_c}"] = functools.partial(group_p, _f, _n, _c, _k)
CASES["P_grid"] = group_grid
CASES["P_slot2_of_3"] = group_p_slot
for _n, _f, _c in l_shapes():
    CASES[f"L_n{_n}_f{_f}_c{_c}"] = functools.partial(group_l, _n, _f, _c)


for _by, _n, _f, _c in E_SHAPES:
    CASES[f"E_{_by}_n{_n}_f{_f}_c{_c}"] = functools.partial(group_e, _by, _n, _f, _c)


def group(letter):
    return [name for name in CASES if name.startswith(letter + "_")]


L_CASES = group("L") + ["P_grid"]         # the grid state serves both kernels


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert c["name"] == name
    return c
