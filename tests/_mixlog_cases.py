"""Values, layouts, reference and bounds for testing the mixture kernels' fp64 logs ENTRY BY ENTRY over the float32 range
(tests/test_mixlog_model_cpu.py, tests/test_gpu_mixture_log_range.py).  Plain NumPy and the standard library; no device.

Every other mixture test compares a sum of hundreds to millions of logs at 1e-10 relative, which cannot see one wrong row
of a log table (1/1024 of the entries), a wrong series coefficient, or an off-by-one at an interval edge.  Here a state
has ONE table entry with a non-zero count (layout A), two (layout B) or one per group tuple (layout C), so a launch's
result is n * log v of a chosen v and is held against np.longdouble's log within a bound derived from the kernel's code.

Values.  float32 probabilities q = m * 2^e: for every one of the 1024 mantissa intervals [1 + i/1024, 1 + (i+1)/1024) of
`tab_log4_n` (sbe_mixture_mfma.hip.h) the lower edge, its float32 successor, the float32 predecessor of the upper edge,
the centre and one seeded interior point, crossed with five exponent classes -- [0.5, 1), [0.25, 0.5), 2^-20, the
smallest float32 normals (2^-126) and the float32 subnormals (2^-127 .. 2^-149, where fewer mantissa bits exist: the
mantissa is truncated to what is representable and duplicates are dropped) -- plus named values.  Every value is a
positive normal double after conversion, so every case is finite.  A mixture value v = sum_c w_c p_c is a convex
combination of probabilities (the weights are normalised per pattern: they are >= 0 and sum to 1 up to float32
rounding), so v >= min_c p_c over the components with non-zero weight: 2^-149, the smallest positive float32, is the
smallest non-zero v any layout can reach.

Reference.  v is restated exactly as the kernels compute it -- the product of two float32 values is exact in fp64, the
sum runs in component order with one rounding per addition -- from the float32 normalised weights of the oracle, and
sum_t n_t log v_t is taken in np.longdouble (64-bit significand: tests/test_mixlog_model_cpu.py holds it against
mpmath at 200 bits to 2^-60 relative).

Model.  `fine_table`, `model_tab_log` and `model_ll` restate the matrix-pipe kernel's log in exact arithmetic (every FMA
one correctly rounded Fraction operation): what the device is expected to return bit for bit in layout A.

Bounds: `matrix_pipe_bound`, `per_obs_bound`, `fuzz_tolerance`; each derivation is in its docstring.
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                                   # half an ulp of 1: |RN(x) - x| <= U |x|
ENTRIES = 1024                                   # kFineLogEntries
SPLIT = 424                                      # kFineLogSplit: 1 + 424/1024 = 1.4140625 ~ sqrt(2)
CARRY = 0x00100000 - (SPLIT << 10)               # kFineLogCarry
BIAS = 1023                                      # kFineLogBias
LN2_D = 6.93147180559945286227e-01               # the kernel's ln 2 (the double next to ln 2)
LN2_REL = 0.31                                   # |LN2_D - ln 2| / ln 2 = 3.35e-17 = 0.30 x 2^-53 (test_mixlog_model_cpu re-measures it)

CLASSES = ("half", "quarter", "2^-20", "min_normal", "subnormal", "named")
_EXP_FIELD = {"half": 126, "quarter": 125, "2^-20": 107, "min_normal": 1}
KINDS = ("lower_edge", "successor", "predecessor_of_upper", "centre", "interior")
SEED = 20261017
# the strided subset of the intervals for the layouts that need several values per state (B, C) and for the sweep over every
# vector-pipe form: every 8th interval, the first two, the last two and both sides of the sqrt(2) split
SUBSET_INTERVALS = tuple(sorted(set(range(0, ENTRIES, 8)) | {0, 1, SPLIT - 1, SPLIT, SPLIT + 1, ENTRIES - 2, ENTRIES - 1}))


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def named_values():
    """[(name, float32 value)]"""
    one = np.float32(1.0)
    r = np.float32(np.sqrt(0.5))                                  # a float32 next to sqrt(1/2); its neighbour on the other side
    lo, hi = (np.nextafter(r, np.float32(0)), r) if float(r) ** 2 > 0.5 else (r, np.nextafter(r, one))
    s = np.float32((1.0 + SPLIT / 1024.0) / 2.0)                  # the split scaled into [0.5, 1): 0.70703125, exact
    return [("1", one), ("nextafter(1,0)", np.nextafter(one, np.float32(0))), ("0.5", np.float32(0.5)),
            ("below sqrt(1/2)", lo), ("above sqrt(1/2)", hi),
            ("below the split", np.nextafter(s, np.float32(0))), ("above the split", np.nextafter(s, one)),
            ("2^-126", np.float32(2.0 ** -126)), ("2^-149", np.float32(2.0 ** -149))]


def values(intervals=None):
    """-> (q float32 [n], cls int [n] index into CLASSES, interval int [n] (of the fp64 image, as the kernel indexes)).
    `intervals`: the mantissa intervals to take (default: all 1024; SUBSET_INTERVALS: the strided subset).  Named values
    first; a grid value equal to a named or an earlier one is dropped (float32 subnormals collapse)."""
    iv = np.arange(ENTRIES, dtype=np.uint32) if intervals is None else np.asarray(intervals, dtype=np.uint32)
    rng = np.random.default_rng(SEED)
    inner = rng.integers(2, (1 << 13) - 1, size=ENTRIES).astype(np.uint32)        # one per interval, whatever the subset
    inner[inner == (1 << 12)] += 1
    lo = iv << 13                                                                   # 23-bit mantissa field of 1 + i/1024
    mant = np.stack([lo, lo + 1, lo + (1 << 13) - 1, lo + (1 << 12), lo + inner[iv]], axis=1)      # [n_iv, 5] in KINDS order
    qs, cs = [np.array([v for _, v in named_values()], dtype=np.float32)], [np.full(len(named_values()), CLASSES.index("named"))]
    for name, field in _EXP_FIELD.items():
        qs.append(_f32((np.uint32(field) << 23) | mant.reshape(-1)))
        cs.append(np.full(mant.size, CLASSES.index(name)))
    # subnormals: m * 2^e, e = -127 .. -149, has e + 149 mantissa bits.  The lower edge takes e = -127 - (i mod 10), where all of
    # its ten interval bits exist (so every interval occurs); the other kinds cycle through all 23 exponents
    kind = np.arange(5, dtype=np.int64)[None, :]
    e = -127 - ((iv.astype(np.int64)[:, None] * 5 + kind) % 23)
    e[:, 0] = -127 - (iv.astype(np.int64) % 10)
    shift = (-126 - e).astype(np.uint32)                                            # bits of the 24-bit significand that do not exist
    sig = ((mant | np.uint32(1 << 23)) >> shift)                                    # truncated: the subnormal's fraction field
    qs.append(_f32(sig.reshape(-1)))
    cs.append(np.full(mant.size, CLASSES.index("subnormal")))
    q, c = np.concatenate(qs), np.concatenate(cs)
    _, first = np.unique(q.view(np.uint32), return_index=True)
    first.sort()
    q, c = q[first], c[first]
    assert np.all(q > 0) and np.all(q <= 1)
    return q, c, interval_of(q.astype(np.float64))


def interval_of(v):
    """Table row of the fp64 value v: bits 51..42 of its mantissa, (hi >> 10) & 1023 in the kernel."""
    return ((np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(42)) & np.uint64(1023)).astype(np.int64)


def reduced_mantissa(v):
    """m' of v = m' 2^K as the kernel splits it: the mantissa in [1, 2), halved from row SPLIT on -> [0.70703125, 1.4140625)."""
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    return np.where(interval_of(v) >= SPLIT, 0.5 * m, m)


# ---- the exact-arithmetic model of tab_log4_n and of the end-of-lane combination --------------------------------------
_TABLE = None


def fine_table():
    """fine_log_table of sbe_mixture_mfma.hip: [1024][2] = {RN(1/c_i) / 2, RN(log c'_i)} with c_0 = 1, c_1023 = 2, else the
    interval's centre; c' = 1 / RN(1/c), halved from row SPLIT on; rows 0 and 1023 hold log = 0 exactly.  In np.longdouble, as
    the host code computes it in long double."""
    global _TABLE
    if _TABLE is None:
        L = np.longdouble
        tab = np.zeros((ENTRIES, 2), dtype=np.float64)
        for i in range(ENTRIES):
            c = L(1) if i == 0 else L(2) if i == ENTRIES - 1 else L(1) + (L(i) + L(0.5)) / L(ENTRIES)
            inv_c = np.float64(L(1) / c)
            lc = -np.log(L(inv_c)) - (np.log(L(2)) if i >= SPLIT else L(0))
            tab[i, 0] = 0.5 * inv_c
            tab[i, 1] = 0.0 if i in (0, ENTRIES - 1) else np.float64(lc)
        _TABLE = tab
    return _TABLE


def _rn(x: Fraction) -> float:
    """Round to nearest even double: CPython's int / int true division is correctly rounded."""
    return x.numerator / x.denominator


_EIGHT_THIRDS = Fraction(8.0 / 3.0)


def model_tab_log(v: float):
    """tab_log4_n on one positive normal double -> (log of the reduced mantissa as the kernel rounds it, biased exponent)."""
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    hi = bits >> 32
    assert 0 < (hi >> 20) < 0x7FF, v
    x, y = fine_table()[(hi >> 10) & 1023]
    m = Fraction(struct.unpack("<d", struct.pack("<Q", (bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0])
    kexp = ((hi + CARRY) & 0xFFFFFFFF) >> 20
    s = Fraction(_rn(m * Fraction(float(x)) - Fraction(1, 2)))
    q = Fraction(_rn(s * -4 + _EIGHT_THIRDS))
    q = Fraction(_rn(s * q - 2))
    q = Fraction(_rn(s * q + 2))
    return _rn(s * q + Fraction(float(y))), kexp


def model_combine(lg: float, kexp: int, n: int) -> float:
    """The kernel's end of lane for ONE entry with count n (read from sbe_mixture_mfma.hip): lsum = fma(n, lg, 0); the integer
    sum n * kexp loses the bias 1023 * (objects of the column) = 1023 n; fma((double)K, ln2, lsum).  Every other term the
    block adds to the slot is an exact zero (entries without counts: fma(0, lg, lsum) = lsum)."""
    lsum = _rn(Fraction(n) * Fraction(lg))
    return _rn(Fraction(n * kexp - BIAS * n) * Fraction(LN2_D) + Fraction(lsum))


def model_ll(v: float, n: int) -> float:
    lg, kexp = model_tab_log(v)
    return model_combine(lg, kexp, n)


# ---- bounds ------------------------------------------------------------------------------------------------------------
A_LOG = 4            # roundings that scale with |log m'| (derivation below)
B_RES = 3            # roundings that scale with |result|


def matrix_pipe_bound(v, n, roundings_of_v=0):
    """Bound on |device - exact| of sum_t n_t log v_t for k_mixture_tuple_mfma; v, n: [..., T] (T entries with counts per
    state; T = 1 in layout A).  u = 2^-53, v = m' 2^K as the kernel splits it, row i.

        per entry     n (D_i + A u |log m'|) + B u |n log v|  [+ n roundings_of_v u],     A = 4, B = 3
        per state     + (T - 1) u sum_t n_t |log m'_t|        (T > 1: the fma(cnt, lg, lsum) chain)
        wide forms    + u sum_t (|n_t log v_t| + n_t |log m'_t|)

    tab_log4_n.  s = fma(m, 1/(2c), -1/2) is r / 2 rounded once (m x has up to 77 bits): relative u.  log m' = y* + log1p(r)
    with y* = log c' exact and y = RN(y*).  The series r - r^2/2 + r^3/3 - r^4/4 drops r^5/5 - r^6/6 + ..: at most
    D_i = r_max^5 / 5 (r_max = 2^-10 in row 0 where c = 1, 2^-11 elsewhere: |m - c| <= 2^-11 and c >= 1; 1.8e-16 and 5.6e-18)
    for r > 0, and for r < 0 that plus |r|^6 / (6 (1 - |r|)) <= 1.001 u |log m'| / 24 (|r|^5 <= 2^-55 = u / 4, |r| <= |log m'|,
    1 / (1 - |r|) <= 1.0005).  The four Horner FMAs: the last one rounds
    the result (u |lg|); the error of s enters as |r| u, the third FMA's rounding (u x 2) as |s| 2u = |r| u, the table's y
    as u |y| <= u (|log m'| + |r|); the first two FMAs' roundings and the rounded 8/3 enter times s^2 <= 2^-24: below
    2^-11 u |r|.  Rows 1 .. 1022: |r| <= |log m'| / 2 (the nearest log is log(1 + 1/1024) = 9.76e-4 against
    |r| <= 2^-11 / c = 4.88e-4; at the top 2^-11 against 2^-12), so the sum is (1 + 1 + 3/2 + 1/24 + ..) u |log m'| < 4 u |log m'|.
    Rows 0 and 1023: y = 0 exactly and |r| <= 1.0005 |log m'|: (1 + 2.001 + 1/24) u |log m'| < 4 u |log m'|.  A = 4.

    End of lane.  lsum = fma(n, lg, 0): u |n lg|.  The exponents are summed as integers, exactly; K ln2 uses the double next
    to ln 2: LN2_REL u |n K ln2|.  The final fma(K, ln2, lsum) rounds once: u |result|.
    No cancellation: a probability has v <= 1, so K <= 0 and K = 0 only for m' <= 1.  Same signs (log m' <= 0): both parts
    are at most |result|.  Opposite signs (log m' > 0, so K <= -1): the split gives log m' < log 1.4140625 = 0.34647 <
    (ln 2) / 2, hence |result| >= |K| ln2 - log m' >= 0.6931 - 0.3465 > log m', and |K ln2| <= |result| + log m' <= 2 |result|.
    So |n lg| <= |result| (1 + small) and |n K ln2| <= 2 |result|: (1 + 2 LN2_REL + 1) u |result| < 3 u |result|.  B = 3.

    Several entries (layouts B, C).  All n_t log v_t are <= 0, so the bounds above add over the entries with |result| the sum.
    The chain lsum = fma(n_t, lg_t, lsum) rounds T times, each time at most u sum_t n_t |log m'_t| (the terms have mixed signs);
    one of those is in B already.  T is taken as the number of entries of the state: every chain is at most that long.
    roundings_of_v: (C - 1) u per log for the roundings of the component sum (d log v = dv / v).
    Wide forms (4 / 2 slots per block): the lane halves hold different tuples; half 0 forms fma(K, ln2, lsum_0) with the
    exponents of BOTH halves (u (|result| + |lsum_1|)) and the halves are added at the end (u |result|); the second of these
    is the final rounding counted in B, the first is the extra line above."""
    L = np.longdouble
    v = np.asarray(v, dtype=np.float64)
    n = np.broadcast_to(np.asarray(n, dtype=np.float64), v.shape)
    row = interval_of(v).reshape(v.shape)
    logm = np.abs(np.log(reduced_mantissa(v).reshape(v.shape).astype(L))).astype(np.float64)
    res = np.abs(n * np.log(v.astype(L))).astype(np.float64)
    D = np.where(row == 0, 2.0 ** -50 / 5.0, 2.0 ** -55 / 5.0)
    return n * (D + A_LOG * U * logm) + B_RES * U * res + n * roundings_of_v * U, n * logm, res


def matrix_pipe_entry_bound(v, n, roundings_of_v=0):
    """Layout A: one entry per state; v, n broadcast -> bound per state."""
    return matrix_pipe_bound(v, n, roundings_of_v)[0]


def matrix_pipe_state_bound(v, n, roundings_of_v=0, wide=False):
    """Layouts B, C: v, n [B, T] -> bound per state [B] (entries with n = 0 count for nothing)."""
    per, t_abs, res = matrix_pipe_bound(v, n, roundings_of_v)
    T = np.count_nonzero(np.broadcast_to(n, np.shape(v)), axis=-1)
    out = per.sum(-1) + np.maximum(T - 1, 0) * U * t_abs.sum(-1)
    if wide:
        out = out + U * (res.sum(-1) + t_abs.sum(-1))
    return out


def per_obs_bound(want, kernel_name, roundings_of_v=0):
    """ONE log per state (N = 1, LOG_PER_OBS) in the vector-pipe forms: the project's own per-log bounds
    (tests/test_gpu_engine.py::test_fast_log_accuracy): 1 ulp for fast_log and the library log, 1.5 ulp + 2^-53 absolute for
    the table log of k_mixture_tuple64; plus the roundings of v.  (Those bounds are against NumPy's fp64 log, itself within
    half an ulp; against the longdouble reference they are no tighter than there.)"""
    want = np.abs(np.asarray(want, dtype=np.float64))
    ulp = np.spacing(want)
    base = 1.5 * ulp + 2.0 ** -53 if "k_mixture_tuple64" in kernel_name else ulp
    return base + roundings_of_v * U


def fuzz_tolerance(want, n_obs):
    """tools/fuzz_gpu.py: 1e-10 relative + 1e-16 per observation (LOG_PRODUCT, and every form at N > 1)."""
    return 1e-10 * np.abs(np.asarray(want, dtype=np.float64)) + 1e-16 * n_obs


# ---- reference ---------------------------------------------------------------------------------------------------------
def log_ref(v):
    return np.log(np.asarray(v, dtype=np.float64).astype(np.longdouble))


def normalized_pair(w):
    """float32 [B, 2] raw weights -> normalised as the oracle does for the pattern (1, 1): w / (w0 + w1), all in float32."""
    w = np.asarray(w, dtype=np.float32)
    return w / (w[:, :1] + w[:, 1:2])


def mix2(w, p0, p1):
    """v = w0 p0 + w1 p1 as the kernels form it: both products exact in fp64, one rounding in the addition."""
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    return w[:, 0] * np.asarray(p0, dtype=np.float32).astype(np.float64) + w[:, 1] * np.asarray(p1, dtype=np.float32).astype(np.float64)


# ---- layouts -----------------------------------------------------------------------------------------------------------
def layout_a(N):
    """F = 1, S = 2, every object observes state 0, one group holding everyone: LL[b] = N log q_b."""
    feats = np.zeros((N, 1, 2), dtype=bool)
    feats[:, 0, 0] = True
    return feats, [1], [np.ones((1, N), dtype=bool)]


def probs_a(q, other_zero):
    p = np.zeros((1, 1, 2), dtype=np.float32)
    p[0, 0, 0] = q
    p[0, 0, 1] = np.float32(0.0) if other_zero else np.float32(1.0) - np.float32(q)
    return p


B_N, B_IN_CLUSTER = 70, 33                       # two k-blocks (64 + 6 objects); roughly half in the cluster


def layout_b():
    """n_groups = [1, 1]: B_IN_CLUSTER of B_N objects in the cluster, the confounder group holds everyone: two tuples, two weight
    patterns -- the shared-operand epilogue.  LL[b] = n_both log(w0' p0 + w1' p1) + n_conf log p1."""
    feats, _, _ = layout_a(B_N)
    cluster = np.zeros((1, B_N), dtype=bool)
    cluster[0, ::2][:B_IN_CLUSTER] = True
    assert cluster.sum() == B_IN_CLUSTER
    return feats, [1, 1], [cluster, np.ones((1, B_N), dtype=bool)]


def cases_b():
    """-> (p0, p1 float32 [n], raw weights float32 [n, 2], class of p0, class of p1): p0 runs through the strided value subset,
    p1 through a seeded permutation of it; the weights cycle through a Dirichlet draw, a float32-subnormal cluster weight
    and a cluster weight of exactly 0 (the confounder's weight must stay positive: its pattern (0, 1) divides by it)."""
    q, c, _ = values(SUBSET_INTERVALS)
    rng = np.random.default_rng(SEED + 1)
    perm = rng.permutation(q.size)
    w = rng.dirichlet(np.ones(2), size=q.size).astype(np.float32)
    k = np.arange(q.size) % 3
    sub = _f32(rng.integers(1, 1 << 23, size=q.size).astype(np.uint32))
    w[k == 1, 0] = sub[k == 1]
    w[k == 2, 0] = 0.0
    assert np.all(w[:, 1] > 0)
    return q, q[perm], w, c, c[perm]


def reference_b(p0, p1, w):
    """-> (v [n, 2], counts [2], LL longdouble [n])"""
    v = np.stack([mix2(normalized_pair(w), p0, p1), np.asarray(p1, dtype=np.float32).astype(np.float64)], axis=1)
    cnt = np.array([B_IN_CLUSTER, B_N - B_IN_CLUSTER], dtype=np.float64)
    return v, cnt, (cnt * log_ref(v)).sum(-1)


C_N = 130
C_WIDTHS = {4: [3, 1, 6], 2: [3, 1, 3, 3]}        # slots per block -> groups per component: up to 28 / 64 tuples
C_SLOTS = 37                                      # no multiple of 4 or 2


def layout_c(n_groups):
    """Objects dealt over every tuple (cluster 0..2 or none) x (every further confounder's group or none); component 1 holds
    everyone.  -> (feats, group masks, tuple id per object, digits [KT, C]: the group of each component, -1 = none)."""
    feats, _, _ = layout_a(C_N)
    radix = [g + 1 if c != 1 else 1 for c, g in enumerate(n_groups)]
    KT = int(np.prod(radix))
    tid = np.arange(C_N) % KT
    digits = np.zeros((KT, len(n_groups)), dtype=np.int64)
    rest = np.arange(KT)
    for c, r in enumerate(radix):
        digits[:, c] = rest % r
        rest = rest // r
    for c, g in enumerate(n_groups):
        if c != 1:
            digits[digits[:, c] == g, c] = -1
    groups = [np.stack([digits[tid, c] == k for k in range(g)]) for c, g in enumerate(n_groups)]
    return feats, groups, tid, digits


def cases_c(n_groups, n_slots=C_SLOTS):
    """Per slot: one value per group row, neighbours in the tuple order from far-apart exponent classes (the class of group row j
    of a component is (j + slot + component) mod 5, so rows that differ in one digit -- tuples t, t + 1, t + 4 .., which share an
    M tile's lane halves -- sit many binary orders apart: 2^-149 beside 0.9), and Dirichlet weights.
    -> (probs: list over components of float32 [n_slots, G_c], weights float32 [n_slots, C])"""
    q, c, _ = values(SUBSET_INTERVALS)
    by_class = [q[c == k] for k in range(5)]
    rng = np.random.default_rng(SEED + 2 + len(n_groups))
    probs = []
    for comp, g in enumerate(n_groups):
        p = np.empty((n_slots, g), dtype=np.float32)
        for b in range(n_slots):
            for j in range(g):
                pool = by_class[(j + b + comp) % 5]
                p[b, j] = pool[rng.integers(0, pool.size)]
        probs.append(p)
    weights = rng.dirichlet(np.ones(len(n_groups)), size=n_slots).astype(np.float32)
    return probs, weights


def reference_c(n_groups, probs, weights, normalize_weights):
    """-> (v [n_slots, KT], counts [KT], LL longdouble [n_slots]); `normalize_weights`: the oracle's (float32)."""
    _, groups, tid, digits = layout_c(n_groups)
    KT, C = digits.shape
    cnt = np.bincount(tid, minlength=KT).astype(np.float64)
    has = digits >= 0                                                            # [KT, C]
    n_slots = weights.shape[0]
    v = np.zeros((n_slots, KT))
    for b in range(n_slots):
        w = normalize_weights(weights[b][None, :], has)[:, 0, :]                 # [KT, C] float32
        for comp in range(C):
            p = np.where(has[:, comp], probs[comp][b][np.maximum(digits[:, comp], 0)], np.float32(1.0))
            term = w[:, comp].astype(np.float64) * p.astype(np.float64)          # exact
            v[b] = term if comp == 0 else v[b] + term                            # one rounding
    return v, cnt, (cnt * log_ref(v)).sum(-1)
