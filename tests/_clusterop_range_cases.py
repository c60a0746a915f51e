"""The range cases of the cluster operators' evaluations (sbayes_amd/csrc/sbe_kernels_operators.hip.h: k_cluster_marginals[_ws],
k_jump_lh[_ws], k_source_lh_by_feature) and their log-space double, shared by tests/test_clusterop_range_cpu.py (which proves
from the double alone that every case is what it claims to be) and tests/test_gpu_clusterop_range.py (device against double).
DESIGN.md section 4.3b.  No GPU import here.

    value_case(C)      C = 8, 5, 2: tests/_srcdraw_range_cases.range_state(C) twice side by side -- its weight columns of exactly 0,
                       1e-42, 2^-126 and 1e30 beside 1e-30 -- with more NA observations, three objects outside every confounder
                       group, one weight row that is exactly (0, 1, 0, ...), and PLANTED float32 tables: candidate, source, target
                       and confounder entries of exactly 0, 1e-42, 2^-126 and exactly 1.  The object list is unsorted and names
                       one object twice.
    edge_state(name)   ordinary make_workload states at F = 1, 63, 64, 65, 255, 256, 257, 513, S = 16, 17, 33, C = 3, 4, 5, 8 and
                       C = 1 (tests/_srcdraw_range_cases.single_component_state).
    limit_state(...)   both sides of the 64 KB table limit of the fused forms.
    slf_entry_state()  N = 1: k_source_lh_by_feature's out[f] is logf of ONE normalised weight.
    slf_edge_state(..) N = 511, 512, 513 x F = 15, 16, 17 with a zero weight at a source, an observation without a source and an
                       all-NA feature.

The double (marginal_v, jump_v, log_terms, row_sums, row_bounds): v of every (object, side, feature) formed exactly like the
device forms it -- float32 weight rows of the oracle, float32 table entries as they stand, for the marginals an explicit fp64
chain v = v + lh_c * w_c over the components in order, for the jump the float32 chain of oracle.jump_lh_per_feature -- then
log v in np.longdouble and the exactly rounded sum of those terms."""
from __future__ import annotations

import contextlib
import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import sbayes_oracle as orc
from sbayes_amd.synthetic import make_workload
from tests._srcdraw_range_cases import DENORMAL, F32, TINY, UNIVERSAL, State, double_of, load, range_state, single_component_state  # noqa: F401

LOG_TINY = math.log(TINY)                        # log 2^-126 = -87.3...
U64 = 2.0 ** -53
POWF = 2e-6                                      # the project's float32 powf allowance per finite term (tests/test_gpu_operators.py)
TEMPERATURES = ((1.3, 1.5), (2.5, 1.7), (1.0, 1.7))
SIZES = (1, 3, 4, 5, 9)                          # n_av / n_members around the four object waves of a wave-specialised block


# ---- the double --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _normalize_unasserted():
    """The oracle's normalize (x / sum(x) in x's dtype, then float32) with the reference's assertion taken out for the length of
    one call: a weight row that sums to 0 must come back as the NaN row the arithmetic gives, which the device computes too --
    with the assertion in place the oracle's weight functions raise for the whole state."""
    kept = orc.normalize

    def plain(x, axis=-1):
        x = np.asarray(x)
        return (x / np.sum(x, axis=axis, keepdims=True)).astype(orc.FLOAT_TYPE)

    orc.normalize = plain
    try:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            yield
    finally:
        orc.normalize = kept


def _f32(a):
    b = np.asarray(a).astype(F32)
    assert np.array_equal(b.astype(np.float64), np.asarray(a, dtype=np.float64), equal_nan=True)    # (float32 values in a wider array)
    return b


def weights_z(st: State, prior_temperature=1.0):
    """float32 [2, N, F, C]: oracle.feature_weights_with_and_without of every object, z = 0 outside / z = 1 inside a cluster."""
    with _normalize_unasserted():
        wz = orc.feature_weights_with_and_without(st.weights, st.has_components, np.ones(st.shape[0], dtype=bool), prior_temperature)
    return _f32(wz)


def weights_heated(st: State, prior_temperature=1.0):
    """float32 [N, F, C]: oracle.weights_heated."""
    with _normalize_unasserted():
        return _f32(orc.weights_heated(st.weights, st.has_components, prior_temperature))


def _ids(st: State):
    """(x int [N, F] with 0 for NA, na bool [N, F], g list of int [N] per component: the object's group or -1)."""
    na = st.na
    x = np.where(na, 0, st.features.argmax(-1))
    g = [np.where(grp.any(axis=0), grp.argmax(axis=0), -1) for grp in st.groups]
    return x, na, g


def _entries(table_gfs, g, x):
    """table[g[i], f, x[i, f]] float32 [n, F] (g < 0: the row of group 0, masked by the caller)."""
    F = x.shape[1]
    return np.asarray(table_gfs, dtype=F32)[np.maximum(g, 0)[:, None], np.arange(F)[None, :], x]


def marginal_v(st: State, probs, table, objects, prior_temperature=1.0, wz=None, drop_na=False):
    """(v float64 [2, n, F], na bool [n, F]): the device's v of every listed object, side and feature.  probs[c], c >= 1: float32
    [G_c, F, S] tables of the other components as they stand; table: float32 [F, S] of the candidate cluster.  NA: lh = 1 in every
    component; a component the object has no group of: 0.  `drop_na`: the wrong kernel that skips NA features (v = 1 there)."""
    objects = np.asarray(objects)
    x, na, g = _ids(st)
    x, na = x[objects], na[objects]
    C = len(st.groups)
    wz = weights_z(st, prior_temperature) if wz is None else wz
    w = wz[:, objects]
    lh = np.empty(x.shape + (C,), dtype=F32)
    lh[..., 0] = _entries(np.asarray(table, dtype=F32)[None], np.zeros(objects.size, dtype=int), x)
    for c in range(1, C):
        gc = g[c][objects]
        lh[..., c] = np.where((gc >= 0)[:, None], _entries(probs[c], gc, x), F32(0))
    lh[na] = 1
    v = np.zeros((2,) + x.shape, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for c in range(C):                                         # v = v + lh_c * w_c: the product exact in fp64, one rounding per addition
            v = v + lh[None, ..., c].astype(np.float64) * w[..., c].astype(np.float64)
    if drop_na:
        v = np.where(na[None], 1.0, v)
    return v, na


def jump_v(st: State, pconf, p_source, p_target, objects, prior_temperature=1.0):
    """(v float64 [2, n, F] holding the float32 stay / jump values, na bool [n, F]): oracle.jump_lh_per_feature's chain on the given
    tables -- float32 multiply, then float32 add, confounder components in order, then the cluster's -- for ANY listed objects.
    pconf: float32 [G_1 + G_2 + ..., F, S]."""
    objects = np.asarray(objects)
    x, na, g = _ids(st)
    x, na = x[objects], na[objects]
    C = len(st.groups)
    wh = weights_heated(st, prior_temperature)[objects]
    pc = np.zeros(x.shape, dtype=F32)
    off = 0
    with np.errstate(invalid="ignore", under="ignore"):
        for c in range(1, C):
            gc = g[c][objects]
            e = _entries(np.asarray(pconf, dtype=F32)[off:off + st.n_groups[c]], gc, x)
            pc = np.where((gc >= 0)[:, None], pc + wh[..., c] * e, pc)
            off += st.n_groups[c]
        zero = np.zeros(objects.size, dtype=int)
        stay = pc + wh[..., 0] * _entries(np.asarray(p_source, dtype=F32).reshape((1,) + x.shape[1:] + (-1,)), zero, x)
        jump = pc + wh[..., 0] * _entries(np.asarray(p_target, dtype=F32).reshape((1,) + x.shape[1:] + (-1,)), zero, x)
    assert stay.dtype == F32 and jump.dtype == F32
    return np.stack([stay, jump]).astype(np.float64), na


def log_terms(v, skip=None):
    """np.longdouble [..]: log v, -inf where v is 0, NaN where v is NaN; exactly 0 where `skip` (the jump's NA features)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(np.asarray(v, dtype=np.float64).astype(np.longdouble))
    if skip is not None:
        t = np.where(np.broadcast_to(skip, t.shape), np.longdouble(0), t)
    return t


def _exact_sum(t):
    """The longdouble terms summed exactly, rounded once to a double."""
    hi = t.astype(np.float64)
    lo = (t - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def row_sums(t):
    """float64 [...]: per row (last axis = features) NaN if a term is NaN, else -inf if one is, else the exact sum."""
    t = np.asarray(t)
    out = np.empty(t.shape[:-1], dtype=np.float64)
    for idx in np.ndindex(*t.shape[:-1]):
        row = t[idx]
        if np.isnan(row).any():
            out[idx] = math.nan
        elif np.isinf(row).any():
            out[idx] = -math.inf
        else:
            out[idx] = _exact_sum(row)
    return out


def additions(F):
    """D: the additions a term passes through in the four kernels -- the per-thread chain over the passes of 256 features, six
    exchange levels of the wave sum, two levels over the four partials."""
    return -(-F // 256) + 8


def row_bounds(t, counted=None, tempered=False):
    """float64 [...]: sum_f 1.5 (ulp(|t_f|) + 2^-53) + D 2^-53 sum_f |t_f| over the finite terms of each row (`counted`: the
    features that contribute a term at all -- every one for the marginals, the observed ones for the jump), plus 2e-6 per
    counted feature when tempered."""
    t = np.asarray(t)
    F = t.shape[-1]
    a = np.abs(t.astype(np.float64))
    fin = np.isfinite(a)
    if counted is not None:
        fin = fin & np.broadcast_to(counted, a.shape)
    a = np.where(fin, a, 0.0)
    per_log = np.where(fin, 1.5 * (np.spacing(a) + U64), 0.0)
    out = per_log.sum(-1) + additions(F) * U64 * a.sum(-1)
    if tempered:
        n = np.broadcast_to(counted, a.shape).sum(-1) if counted is not None else F
        out = out + POWF * n
    return out


def pattern(x):
    """0 finite, 1 -inf, 2 NaN, 3 anything else (+inf), elementwise."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 2, np.where(np.isneginf(x), 1, np.where(np.isfinite(x), 0, 3)))


# ---- 1: the value range --------------------------------------------------------------------------------------------------------
@dataclass
class ValueCase:
    st: State
    objects: np.ndarray             # int32, unsorted, one object twice
    probs: list                     # per component float32 [G_c, F, S] (index 0: None): the marginals' other components
    table: np.ndarray               # float32 [F, S] candidate cluster
    pconf: np.ndarray               # float32 [G_1 + ..., F, S]: the jump's confounder tables
    p_source: np.ndarray
    p_target: np.ndarray
    special: dict                   # feature and object sets of the planted rows


def _own_tables(st: State):
    """The state's own float32 tables: [None, probs_1, ...], candidate (cluster 0), target (cluster 1)."""
    C = len(st.groups)
    probs = [None] + [orc.component_probs(st.counts[c], st.conc[c]) for c in range(1, C)]
    clusters = orc.component_probs(st.counts[0], st.conc[0])
    return probs, clusters[0].copy(), clusters[1 % clusters.shape[0]].copy()


@functools.lru_cache(maxsize=None)
def value_case(C):
    base = range_state(C)
    N, F0, _ = base.shape
    S = base.features.shape[2]
    rng = np.random.default_rng(200 + C)
    two = lambda a, axis: np.concatenate([a, a], axis=axis)                                  # noqa: E731
    features = two(base.features, 1)
    features[rng.random(features.shape[:2]) < 0.06] = False                                  # more NA observations
    groups = [g.copy() for g in base.groups]
    K = groups[0].shape[0]
    for n in np.flatnonzero(~groups[0].any(axis=0))[::2]:                                    # three of four objects are cluster members
        groups[0][n % K, n] = True
    members = np.flatnonzero(groups[0].any(axis=0))
    loners = np.flatnonzero(~groups[0].any(axis=0))
    outside = np.array([members[0], members[1], loners[0]])                                  # outside every confounder group
    for c in range(1, C):
        groups[c][:, outside] = False
    pool = rng.permutation(np.setdiff1d(members, outside))
    assert pool.size >= 26, pool.size
    one_side, both_sides, tiny = pool[:10], pool[10:14], pool[14:26]
    ones = pool[6:]                                                                          # (the one-hot weight row: v = 1)
    fa, fb, fc, fd, fe = F0, F0 + 6, F0 + 12, F0 + 18, F0 + 2                                # weight pattern 0 (ordinary) but fe
    weights = two(base.weights, 0)
    weights[fe] = 0
    weights[fe, UNIVERSAL] = 0.75                                                            # normalises to exactly (0, 1, 0, ...)
    for f, who in ((fa, one_side), (fb, both_sides), (fc, tiny), (fd, tiny), (fe, ones)):
        seen = features[:, f].any(axis=-1)
        features[seen, f] = np.eye(S, dtype=bool)[1]                                         # everybody observes state 1 ...
        features[who, f] = np.eye(S, dtype=bool)[0]                                          # ... but the chosen, who observe state 0
    if C == 2:
        # two normalised float32 weights nearly always add up to exactly 1 in fp64 (an NA term of exactly 0 says nothing): two
        # features get weights chosen so that they do not, and more than half of the objects are NA there
        for f in (F0 + 1, F0 + 3):
            while True:
                a = rng.random(2).astype(F32)
                t = a[0] + a[1]
                if float(a[0] / t) + float(a[1] / t) != 1.0:
                    break
            weights[f] = a
            features[rng.permutation(N)[:N // 2 + 5], f] = False
    source = two(base.source, 1)
    source[~features.any(axis=-1)] = False
    st = State(name=f"value{C}", features=features, groups=groups, conc=[two(c, c.ndim - 2) for c in base.conc], weights=weights,
               source=source, unif=two(base.unif, 0))
    probs, table, p_target = _own_tables(st)
    p_source = table.copy()
    kinds = (F32(0), F32(DENORMAL), F32(TINY), F32(1))
    # scattered: state 1 of the features of the first half, one group per confounder; the universal table never 0 (it keeps v > 0)
    for f in range(F0):
        for c in range(2, C):
            probs[c][0, f, 1] = kinds[(f + c) % 4]
        if f % 8 in (5, 7):
            probs[UNIVERSAL][0, f, 1] = kinds[1] if f % 8 == 5 else kinds[3]
        if f % 5:
            table[f, 1] = p_source[f, 1] = kinds[f % 5 - 1]
        if (f + 2) % 5:
            p_target[f, 1] = kinds[(f + 2) % 5 - 1]
    # planted rows: state 0 of five features of the second half, every group of every confounder alike
    for c in range(1, C):
        probs[c][:, fa, 0] = probs[c][:, fb, 0] = 0
        probs[c][:, fc, 0] = DENORMAL
        probs[c][:, fd, 0] = TINY
        probs[c][:, fe, 0] = 1
    table[fa, 0], p_source[fa, 0], p_target[fa, 0] = 0.25, 0.25, 0                           # -inf outside the cluster / for the jump only
    table[fb, 0] = p_source[fb, 0] = p_target[fb, 0] = 0                                     # -inf on both sides
    table[fc, 0], p_source[fc, 0], p_target[fc, 0] = DENORMAL, DENORMAL, TINY
    table[fd, 0], p_source[fd, 0], p_target[fd, 0] = TINY, TINY, DENORMAL
    table[fe, 0] = p_source[fe, 0] = p_target[fe, 0] = 1
    objects = rng.permutation(N).astype(np.int32)
    objects = np.insert(objects, N // 2, objects[3])                                         # unsorted, one object twice
    for a in (*probs[1:], table, p_source, p_target):
        a.setflags(write=False)
    return ValueCase(st=st, objects=objects, probs=probs, table=table, pconf=np.concatenate(probs[1:]), p_source=p_source,
                     p_target=p_target, special=dict(fa=fa, fb=fb, fc=fc, fd=fd, fe=fe, one_side=one_side, both_sides=both_sides,
                                                     tiny=tiny, ones=ones, outside=outside))


# ---- 2: shape edges ------------------------------------------------------------------------------------------------------------
#              N    F   S   K  extra               ragged
EDGE_SHAPES = {
    "f1":    (70,   1,  3, 2, (2,),                False),     # C = 3; one feature: 255 idle threads
    "f63":   (70,  63,  4, 2, (2, 2),              True),      # C = 4: the most the fused forms hold
    "f64":   (70,  64, 16, 2, (2,),                False),     # S = 16: probs_row's register cap
    "f65":   (70,  65, 17, 2, (2,),                True),      # S = 17: the general row form; one feature in the second wave
    "f255":  (70, 255,  3, 2, (2, 2, 2),           False),     # C = 5: block form only
    "f256":  (70, 256,  4, 2, (2,),                False),     # one full pass
    "f257":  (70, 257,  3, 2, (2, 2, 2, 2, 2, 2),  False),     # C = 8; the second pass holds one feature
    "f513":  (70, 513,  2, 2, (2,),                True),      # the third pass holds one feature
    "s33":   (70,  20, 33, 2, (2,),                True),      # S = 33
}


@functools.lru_cache(maxsize=None)
def edge_state(name):
    if name == "c1":
        return single_component_state()
    wl = make_workload(f"clusterop_{name}", shape=EDGE_SHAPES[name])
    return State(name=name, features=wl.features.copy(), groups=[g.copy() for g in wl.groups], conc=[c.copy() for c in wl.concentration],
                 weights=wl.weights.copy(), source=wl.source.copy(), unif=wl.states_per_feature.astype(np.float64))


def member_lists(st: State, seed):
    """(i_source, i_target, {size: int32 list}): the source cluster with the most members and unsorted lists of 1, 3, 4, 5, 9 of them."""
    sizes = st.groups[0].sum(axis=1)
    i_source = int(sizes.argmax())
    members = np.flatnonzero(st.groups[0][i_source])
    assert members.size >= max(SIZES), (st.name, members.size)
    rng = np.random.default_rng(seed)
    return i_source, (i_source + 1) % st.groups[0].shape[0], {n: rng.permutation(members)[:n].astype(np.int32) for n in SIZES}


def available_lists(st: State, i_cluster, seed):
    """{size: int32 list} of objects in cluster i_cluster or in none (what AlterCluster lists), unsorted."""
    av = np.flatnonzero(~st.groups[0].any(axis=0) | st.groups[0][i_cluster])
    rng = np.random.default_rng(seed)
    return {n: rng.permutation(av)[:n].astype(np.int32) for n in SIZES}


# ---- 3: the fused forms' table limit ---------------------------------------------------------------------------------------------
LIMIT_BYTES = 65536
LIMITS = {                       # kind, shape, confounders kept, table bytes
    "marginals-512": ("marginals", (8, 512, 32, 2, (), False)),              # F S 4 = 65536: fused
    "marginals-513": ("marginals", (8, 513, 32, 2, (), False)),              # 65664: table kernel in front
    "jump-7-7":      ("jump", (24, 64, 16, 2, (7, 7), False)),               # (2 + 14) F S 4 = 65536: fused
    "jump-7-8":      ("jump", (24, 64, 16, 2, (7, 8), False)),               # (2 + 15) F S 4 = 69632: three table kernels in front
}


@functools.lru_cache(maxsize=None)
def limit_state(name):
    """(state, table bytes of the fused form).  The jump states have the clusters and two confounders of 7 and 7 (8) groups and
    NO universal component, so that the confounder groups number 14 (15); an observation whose source was the universal
    component has none."""
    kind, shape = LIMITS[name]
    wl = make_workload(f"clusterop_{name}", shape=shape)
    N, F, S = wl.features.shape
    if kind == "marginals":
        st = State(name=name, features=wl.features.copy(), groups=[g.copy() for g in wl.groups], conc=[c.copy() for c in wl.concentration],
                   weights=wl.weights.copy(), source=wl.source.copy(), unif=wl.states_per_feature.astype(np.float64))
        return st, F * S * 4
    keep = [0, 2, 3]
    groups = [wl.groups[c].copy() for c in keep]
    st = State(name=name, features=wl.features.copy(), groups=groups, conc=[wl.concentration[c].copy() for c in keep],
               weights=wl.weights[:, keep].copy(), source=wl.source[:, :, keep].copy(), unif=wl.states_per_feature.astype(np.float64))
    return st, (2 + sum(st.n_groups[1:])) * F * S * 4


# ---- 4: k_source_lh_by_feature -----------------------------------------------------------------------------------------------------
SLF_F = 4000


@functools.lru_cache(maxsize=None)
def slf_entry_state():
    """N = 1, C = 2, one object in cluster 0 and in the universal group, S = 2.  Feature f has weights (a, 1) or (1, a) with a
    from 2^-149 to 2^127 in steps of a fifteenth of a binade or so, and the source alternates between the two components: the
    normalised weight at the source runs from denormals over 1/2 to 1 - 2^-24 and exactly 1."""
    F = SLF_F
    rng = np.random.default_rng(40)
    features = np.zeros((1, F, 2), dtype=bool)
    features[0, np.arange(F), np.arange(F) % 2] = True
    a = np.exp2(np.linspace(-149, 127, F) + rng.uniform(-0.03, 0.03, F)).astype(F32)
    a[0] = 2.0 ** -149
    weights = np.ones((F, 2), dtype=F32)
    weights[np.arange(F), (np.arange(F) // 2) % 2] = a
    source = np.zeros((1, F, 2), dtype=bool)
    source[0, np.arange(F), (np.arange(F) // 4) % 2] = True
    unif = np.ones((F, 2))
    return State(name="slf1", features=features, groups=[np.ones((1, 1), dtype=bool), np.ones((1, 1), dtype=bool)],
                 conc=[unif.copy(), unif[None].copy()], weights=weights, source=source, unif=unif)


SLF_EDGES = tuple((n, f) for n in (511, 512, 513) for f in (15, 16, 17))


@functools.lru_cache(maxsize=None)
def slf_edge_state(N, F):
    """An ordinary state whose feature 0 has weight exactly 0 in the confounder component (some observation's source), whose
    observation (N - 1, F - 1) has no source set, and whose feature 1 (F > 2) is NA in every object."""
    wl = make_workload(f"clusterop_slf_{N}_{F}", shape=(N, F, 3, 2, (2,), False))
    features, source, weights = wl.features.copy(), wl.source.copy(), wl.weights.copy()
    weights[0, 2] = 0
    n = int(np.flatnonzero(wl.groups[2].any(axis=0) & features[:, 0].any(axis=-1))[0])
    source[n, 0] = (False, False, True)                        # the zero weight IS some observation's source
    features[N - 1, F - 1] = (True, False, False)
    source[N - 1, F - 1] = False
    features[:, 1] = False
    source[:, 1] = False
    return State(name=f"slf_{N}_{F}", features=features, groups=[g.copy() for g in wl.groups], conc=[c.copy() for c in wl.concentration],
                 weights=weights, source=source, unif=wl.states_per_feature.astype(np.float64))


def slf_selected(st: State):
    """float32 [N, F]: the normalised weight of each observation's source component; 0 where none is set, 1 where NA."""
    with np.errstate(invalid="ignore", divide="ignore"):
        w = orc.normalize_weights(st.weights, st.has_components)
    assert w.dtype == F32
    ids = st.source_ids
    C = w.shape[-1]
    p = np.take_along_axis(w, np.minimum(ids, C - 1)[..., None].astype(np.int64), axis=-1)[..., 0]
    p = np.where(ids < C, p, F32(0))
    return np.where(st.na, F32(1), p).astype(F32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def slf_double(st: State):
    """(want float64 [F]: math.fsum of the exact logs, -inf as soon as one selected weight is 0; bound float64 [F]:
    sum_n ulp32(term) + 7 2^-53 sum |term| + 1/2 ulp32(result))."""
    p = slf_selected(st).astype(np.float64)
    with np.errstate(divide="ignore"):
        t = np.log(p.astype(np.longdouble)).astype(np.float64)          # (the double's own rounding: 2^-53 relative, against ulp32)
    F = p.shape[1]
    want, bound = np.empty(F), np.empty(F)
    for f in range(F):
        col = t[:, f]
        if np.isinf(col).any():
            want[f], bound[f] = -math.inf, 0.0
            continue
        want[f] = math.fsum(col)
        bound[f] = ulp32(col[col != 0]).sum() + 7 * U64 * np.abs(col).sum() + 0.5 * float(ulp32(want[f]))
    return want, bound
