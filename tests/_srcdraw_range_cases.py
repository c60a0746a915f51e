"""The range cases of the Gibbs source draw (sbayes_amd/csrc/sbe_kernels_sampling.hip.h: "posterior row over the components,
float32 cdf, first component whose cdf exceeds the uniform" in its three hand-written forms), shared by
tests/test_srcdraw_range_cpu.py (which asserts with the oracle-backed double alone that every case is what it claims to be) and
tests/test_gpu_srcdraw_range.py (device against the double).  DESIGN.md section 4.3a.  No GPU import here.

    range_state(C)     C = 8, 5, 2: weight columns overwritten by exactly 0, a float32 denormal, the smallest normal and a
                       1e30 / 1e-30 spread within one row; two cluster concentration columns so small that the float32 table
                       entry of an unseen state is 0 or denormal; confounders some objects have no group of; NA observations.
    plant(p, seed)     uniforms ON the steps of the double's own float32 cdf, one double below them, at 0, at 1 - 2^-53, on
                       steps tied by zero-probability components and on a first step that is 0.
    plant_clear(p, .)  uniforms 1e-4 (and a little) from a step: what a tempered device row must still decide like the double.
    logq_state()       a current source that points at components of probability exactly 0: log_q_back = -inf.
    fail_state(k)      exactly k observations, in different blocks and feature tiles, whose every component has likelihood x
                       weight 0 (pure zeros, no NaN), next to the repaired state on the same feature block.
    edge_state(name)   ordinary make_workload states at the block, tile and table-path edges of the kernels; C = 1.

A state is a `State`; `load(engine, state)` puts it into slot 0 of the device engine or of the double alike."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import sbayes_oracle as orc
from sbayes_amd.synthetic import Workload, make_workload
from tests._fake_engine import FakeEngine

F32 = np.float32
TINY = float(np.finfo(F32).tiny)                 # the smallest float32 normal, 2^-126
DENORMAL = 1e-42                                 # a float32 denormal (300 steps of 2^-149 or so)
TOP = 1.0 - 2.0 ** -53                           # the largest uniform a 53-bit generator returns
NEAR = 1e-5                                      # a tempered draw may differ from the double's within this of a step
CLEAR = 1e-4                                     # ... and planted tempered uniforms keep this distance
TEMPERATURES = ((1.3, 1.5), (2.5, 1.7), (1.0, 1.7), (2.5, 1.0))


@dataclass
class State:
    name: str
    features: np.ndarray            # bool [N, F, S]
    groups: list                    # per component bool [G_c, N]
    conc: list                      # per component float64 [F, S] / [G_c, F, S]
    weights: np.ndarray             # float32 [F, C]
    source: np.ndarray              # bool [N, F, C]
    unif: np.ndarray                # float64 [F, S]
    counts: list = None             # per component float32 [G_c, F, S]: the source's own counts

    def __post_init__(self):
        self.weights = np.ascontiguousarray(self.weights, dtype=F32)
        if self.counts is None:
            self.counts = orc.recalculate_feature_counts(self.features, self.groups, self.source)
        for a in (self.features, self.weights, self.source, self.unif, *self.groups, *self.conc, *self.counts):
            a.setflags(write=False)

    @property
    def n_groups(self):
        return [g.shape[0] for g in self.groups]

    @property
    def shape(self):
        return self.source.shape                                  # (N, F, C)

    @property
    def na(self):
        return ~self.features.any(axis=-1)

    @property
    def has_components(self):
        return orc.has_components(self.groups)

    @property
    def source_ids(self):
        return np.where(self.source.any(-1), self.source.argmax(-1), 255).astype(np.uint8)


def _state_of(name, wl: Workload, **changed):
    parts = dict(features=wl.features.copy(), groups=[g.copy() for g in wl.groups], conc=[c.copy() for c in wl.concentration],
                 weights=wl.weights.copy(), source=wl.source.copy(), unif=wl.states_per_feature.astype(np.float64))
    parts.update(changed)
    return State(name=name, **parts)


def load(engine, st: State, slot=0):
    """The state into `slot` of a device engine or of the double, as tests/test_gpu_delta_forms.py's _pair loads both."""
    C = len(st.groups)
    for c in range(C):
        engine.set_concentration(c, st.conc[c])
        engine.set_groups(slot, c, st.groups[c])
        engine.set_counts(slot, c, st.counts[c])
    engine.set_source(slot, st.source)
    engine.set_weights(slot, st.weights)
    engine.set_uniform_counts(st.unif)
    for c in range(C):
        engine.update_probs(slot, c)
    return engine


def double_of(st: State):
    return load(FakeEngine(st.features, st.n_groups), st)


def ids_of(rows):
    """Source rows bool [n, F, C] -> component id uint8 [n, F], 255 where none is set."""
    return np.where(rows.any(-1), rows.argmax(-1), 255).astype(np.uint8)


def fsum_log(sel, na):
    """The sum the device promises for log_q: float64 logs of the float32 selected probabilities, NA observations
    contributing 0, summed exactly (-inf as soon as a selected probability is 0)."""
    v = np.asarray(sel, dtype=np.float64)[~na]
    if (v == 0).any():
        return -math.inf
    return math.fsum(math.log(x) for x in v)


# ---- 1: the probability range ------------------------------------------------------------------------------------------------
RANGE_SHAPES = {8: (50, 24, 3, 2, (2, 2, 2, 2, 2, 2), True),      # C = 8: NumPy sums eight terms by its eight-accumulator tree
                5: (70, 40, 4, 2, (2, 3, 2), True),                # C = 5: more components than the fused kernels hold in registers
                2: (60, 33, 5, 3, (), True)}                       # C = 2: clusters (half of the objects in none) and the universal one
UNIVERSAL = 1                                                      # (every object is in its one group: its weight stays positive)


@functools.lru_cache(maxsize=None)
def range_state(C):
    """Feature f takes weight pattern f % 6: ordinary | one component exactly 0 | one a denormal | one the smallest normal | one
    1e30 next to one 1e-30 u (the others fall to 1e-31 of the row, the small one to exactly 0) | one 0 and one denormal.  The
    universal component keeps a weight that normalises to something positive, so no row of the posterior is all zero."""
    wl = make_workload(f"srcdraw_range{C}", shape=RANGE_SHAPES[C])
    rng = np.random.default_rng(100 + C)
    w = wl.weights.copy()
    F = w.shape[0]
    others = [c for c in range(C) if c != UNIVERSAL]
    for f in range(F):
        pick = [others[i] for i in rng.permutation(len(others))]
        a, b = pick[0], pick[1 % len(pick)]
        kind = f % 6
        if kind == 1:
            w[f, a] = 0.0
        elif kind == 2:
            w[f, a] = DENORMAL
        elif kind == 3:
            w[f, a] = TINY
        elif kind == 4:
            if C == 2:
                w[f, UNIVERSAL], w[f, a] = 1e30, 1e-30 * rng.random()
            else:
                w[f, a], w[f, b] = 1e30, 1e-30 * rng.random()
        elif kind == 5:
            w[f, a] = 0.0
            if b != a:
                w[f, b] = DENORMAL
            else:
                w[f, UNIVERSAL] = DENORMAL                         # (C = 2: the row (0, denormal) normalises to (0, 1))
    conc = [c.copy() for c in wl.concentration]
    n_states = wl.states_per_feature.sum(axis=1)
    conc[0][:, 0] = 1e-46                                          # an unseen state 0 of a cluster: table entry exactly 0
    conc[0][n_states >= 3, 1] = 3e-42                              # ... an unseen state 1: a denormal entry (where a third state keeps
    return _state_of(f"range{C}", wl, weights=w, conc=conc)        #     the tempered row positive: 1 + (3e-42 - 1) is 0 in float64)


def zero_and_denormal_share(p):
    p = np.asarray(p)
    return float((p == 0).mean()), float(((p > 0) & (p < TINY)).mean())


# ---- 2: planted uniforms -----------------------------------------------------------------------------------------------------
KINDS = ("on", "below", "zero", "top", "tie", "tie_top", "cdf0")
ON, BELOW, ZERO, TOPK, TIE, TIE_TOP, CDF0 = range(7)


def steps_of(p):
    """The steps sample_categorical (oracle/sbayes_oracle.py) compares the uniform with: cumulative sums in p's dtype / the last."""
    cdf = np.cumsum(p, axis=-1)
    cdf /= cdf[..., [-1]]
    return cdf


def plant(p, seed):
    """(z float64 [n, F], kind int [n, F], c int [n, F]): one planted uniform per observation of the rows p [n, F, C].
        on       z = float64(cdf[c]) < 1: the draw is the NEXT component of positive probability (z < cdf[c] is false); C = 1:
                 z = 1.0, the only step, and component 0 by the rule of tie_top
        below    z = nextafter(float64(cdf[c]), -1), cdf[c] > 0: the component that carries the cdf up to cdf[c]
        zero     z = 0.0, cdf[0] > 0: component 0
        top      z = 1 - 2^-53: the component that carries the cdf to 1, never a zero-probability one behind it
        tie      z = float64(cdf[c]), cdf[c] == cdf[c + 1] < 1: the zero-probability component c + 1 is stepped over
        tie_top  z = float64(cdf[c]) = 1.0, cdf[c] == cdf[c + 1]: ON the top step nothing exceeds z -- component 0 by
                 sample_categorical's argmax of an all-False row (z = 1 is outside [0, 1): the one planted kind whose draw
                 may have probability 0)
        cdf0     z = 0.0 = float64(cdf[0]): component 0 has probability 0 and is stepped over
    Scarce kinds (ties, a zero first step) are served first, the rest of the observations alternate on / below with c
    running over the components."""
    cdf = steps_of(p)
    n, F, C = p.shape
    rng = np.random.default_rng(seed)
    z = np.empty((n, F), dtype=np.float64)
    kind = np.full((n, F), -1, dtype=np.int64)
    comp = np.zeros((n, F), dtype=np.int64)
    cdf64 = cdf.astype(np.float64)
    quota = max(20, (n * F) // 10)
    order = rng.permutation(n * F)
    taken = np.zeros(n * F, dtype=bool)

    def serve(k, eligible, value, c_of=None):
        """Give kind k to up to `quota` untaken observations of the flat mask `eligible`."""
        idx = [i for i in order if eligible[i] and not taken[i]][:quota]
        for i in idx:
            r, f = divmod(int(i), F)
            cc = int(c_of(r, f)) if c_of is not None else 0
            z[r, f], kind[r, f], comp[r, f] = value(r, f, cc), k, cc
            taken[i] = True

    tied = (cdf[..., :-1] == cdf[..., 1:]) if C > 1 else np.zeros((n, F, 0), dtype=bool)
    low_tie = tied & (cdf[..., :-1] < 1)
    top_tie = tied & (cdf[..., :-1] == 1)
    first = lambda mask: (lambda r, f: np.flatnonzero(mask[r, f])[0])                    # noqa: E731
    serve(TIE, low_tie.any(-1).ravel(), lambda r, f, c: cdf64[r, f, c], first(low_tie))
    serve(TIE_TOP, top_tie.any(-1).ravel(), lambda r, f, c: cdf64[r, f, c], first(top_tie))
    serve(CDF0, (cdf[..., 0] == 0).ravel(), lambda r, f, c: 0.0)
    serve(TOPK, top_tie.any(-1).ravel(), lambda r, f, c: TOP)                            # (rows with zero-probability components at the end first)
    serve(TOPK, np.ones(n * F, dtype=bool), lambda r, f, c: TOP)
    serve(ZERO, (cdf[..., 0] > 0).ravel(), lambda r, f, c: 0.0)
    for i in np.flatnonzero(~taken):
        r, f = divmod(int(i), F)
        want_on = (i // C) % 2 == 0
        for step in range(C):                                      # c runs over the components with the observation index
            c = (int(i) + step) % C
            if want_on and cdf[r, f, c] < 1:
                z[r, f], kind[r, f], comp[r, f] = cdf64[r, f, c], ON, c
                break
            if not want_on and cdf[r, f, c] > 0:
                z[r, f], kind[r, f], comp[r, f] = np.nextafter(cdf64[r, f, c], -1.0), BELOW, c
                break
        else:                                                      # (cdf = [1, ..., 1] asked for `on`: the only step there is, 1.0)
            z[r, f], kind[r, f], comp[r, f] = 1.0, (ON if C == 1 else TIE_TOP), 0
    assert (kind >= 0).all() and (z >= 0).all() and (z <= 1).all()
    return z, kind, comp


def distance_to_steps(p, z):
    """|z - nearest step of the double's cdf|, float64 [n, F]."""
    return np.abs(steps_of(p).astype(np.float64) - np.asarray(z, dtype=np.float64)[..., None]).min(axis=-1)


def plant_clear(p, seed):
    """Uniforms for a TEMPERED row: in a gap of the double's cdf (0 counts as its lower end) at least 4e-4 wide, 1e-4 and a
    random 0 .. 1e-5 more from one of the gap's two ends -- ten times the distance within which a device draw may differ, so
    none of them is excluded from the comparison."""
    cdf = steps_of(p).astype(np.float64)
    n, F, C = p.shape
    rng = np.random.default_rng(seed)
    edges = np.concatenate([np.zeros((n, F, 1)), cdf], axis=-1)
    width = np.diff(edges, axis=-1)                                # [n, F, C]: gap c lies below step c
    z = np.empty((n, F), dtype=np.float64)
    for r in range(n):
        for f in range(F):
            wide = np.flatnonzero(width[r, f] >= 4 * CLEAR)
            c = int(wide[(r * F + f) % wide.size])
            off = CLEAR * (1.0 + 0.1 * rng.random())
            z[r, f] = edges[r, f, c] + off if (r + f) % 2 == 0 else edges[r, f, c + 1] - off
    return z


# ---- the cluster operators' form: has_components rows of two samples, old source, group ids ---------------------------------------
def gu_inputs(st: State, objs, seed):
    """What given_unchanged_gibbs is handed for the sorted subset `objs`: (hc_new, hc_old, src_old, gid_old, gid_new).  hc_new is
    the state's own; in the OLD sample every other object of the subset had the opposite cluster bit (cluster 0 where it had
    one); an old source that names the cluster component without a cluster names the universal one instead."""
    objs = np.asarray(objs)
    rng = np.random.default_rng(seed)
    C = len(st.groups)
    off = np.concatenate([[0], np.cumsum(st.n_groups)]).astype(int)
    hc_new = st.has_components[objs].copy()
    hc_old = hc_new.copy()
    flip = np.zeros(objs.size, dtype=bool)
    flip[rng.permutation(objs.size)[: (objs.size + 1) // 2]] = True
    if C > 1:                                                      # (C = 1: an object without its only component has no weight row)
        hc_old[flip, 0] = ~hc_old[flip, 0]
    gid_new = np.stack([np.where(st.groups[c][:, objs].any(axis=0), st.groups[c][:, objs].argmax(axis=0) + off[c], -1)
                        for c in range(C)]).astype(np.int32)
    gid_old = gid_new.copy()
    gid_old[0] = np.where(hc_old[:, 0], np.where(hc_new[:, 0], gid_new[0], 0), -1)
    src_old = st.source_ids[objs].copy()
    if C > 1:
        src_old[(src_old == 0) & ~hc_old[:, [0]].repeat(src_old.shape[1], 1)] = UNIVERSAL
    return hc_new, hc_old, src_old, gid_old, gid_new


# ---- 5: log_q_back = -inf ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logq_state():
    """range_state(5) with the source of every observation whose posterior row has an exactly-zero component the object is in
    (a zero weight, an unseen state under the tiny concentration) moved onto that component: the backward probability of a
    proposal from this state, and source_logprob at this source, select 0 there."""
    st = range_state(5)
    fake = double_of(st)
    N, F, C = st.shape
    p = fake.source_posterior(0, np.arange(N))
    hc = st.has_components
    zero_here = (p == 0) & hc[:, None, :] & ~st.na[..., None]
    source = st.source.copy()
    rows = zero_here.any(-1)
    source[rows] = np.eye(C, dtype=bool)[zero_here.argmax(-1)[rows]]
    return State(name="logq", features=st.features.copy(), groups=[g.copy() for g in st.groups], conc=[c.copy() for c in st.conc],
                 weights=st.weights.copy(), source=source, unif=st.unif.copy())


# ---- 6: normalize fails ------------------------------------------------------------------------------------------------------
FAIL_SHAPE = (40, 40, 4, 2, (3,), False)                          # C = 3 (clusters, universal, one confounder), three feature tiles
FAIL_SPOTS = ((29, 37), (0, 3), (12, 20))                         # (subset row, feature): blocks 4, 0, 1 of 256 observations; tiles 2, 0, 1
FAIL_N_SUB = 30


@functools.lru_cache(maxsize=None)
def fail_state(k):
    """(bad, good, objs, spots): in `bad`, observation (objs[r], f) of each of the first k FAIL_SPOTS is the only one of
    feature f in the LAST state; feature f's weights are (1/2, 1/2, 0); the cluster prior and the universal prior give that
    state concentration 0, and no observation of it has the cluster or the universal component as its source (the spot's own
    is the confounder) -- so both tables hold exactly 0 there and the confounder's weight is 0: likelihood x weight is 0 in
    every component, by zeros alone.  The kept-observations tables of the cluster operators agree: 1 + (0 - 1) = 0.
    `good` is the same feature block with ordinary weights and concentrations.  The objects of the spots are in a cluster and
    in a confounder group; objs lists 30 objects (1200 observations, five blocks), ascending."""
    wl = make_workload("srcdraw_fail", shape=FAIL_SHAPE)
    N, F, S = wl.features.shape
    last = S - 1
    objs = np.sort(np.random.default_rng(6).choice(N, size=FAIL_N_SUB, replace=False)).astype(np.int32)
    spots = FAIL_SPOTS[:k]
    features, source, groups = wl.features.copy(), wl.source.copy(), [g.copy() for g in wl.groups]
    weights, conc = wl.weights.copy(), [c.copy() for c in wl.concentration]
    for r, f in spots:
        n = int(objs[r])
        for c in (0, 2):                                           # the object is in a cluster and in a confounder group
            if not groups[c][:, n].any():
                groups[c][0, n] = True
        moved = features[:, f, last].copy()                        # everybody else leaves the last state of feature f
        features[moved, f, 0] = True
        features[moved, f, last] = False
        features[n, f] = False
        features[n, f, last] = True
        weights[f] = (0.5, 0.5, 0.0)
        source[n, f] = (False, False, True)
        conc[0][f, last] = 0.0
        conc[1][0, f, last] = 0.0
    good = _state_of(f"fail{k}_good", wl, features=features.copy(), source=source.copy(), groups=[g.copy() for g in groups])
    bad = _state_of(f"fail{k}_bad", wl, features=features, source=source, groups=groups, weights=weights, conc=conc)
    return bad, good, objs, spots


# ---- 7: shape edges ------------------------------------------------------------------------------------------------------------
#            N    F   S  K  extra   ragged      subset sizes (n_sub F: the block edge of the 256-thread kernels; n_sub 16: the tile block)
EDGE_SHAPES = {
    "f1":  ((260, 1, 3, 2, (2,), False),        (1, 128, 129, 255, 256, 257)),   # n_sub F = 1, 255, 256, 257; the proposal's tile form up to 128 objects
    "f15": ((70, 15, 8, 2, (2,), False),        (1, 17, 64, 65)),         # S = 8: eight lanes per table row; 17 x 15 = 255
    "f16": ((70, 16, 9, 2, (2,), False),        (1, 16, 64, 65)),         # S = 9: sixteen lanes per row; 16 x 16 = 256; a full tile
    "f17": ((70, 17, 16, 2, (2,), True),        (1, 15, 64, 65)),         # S = 16; 15 x 17 = 255; one feature in the second tile
    "f33": ((70, 33, 17, 2, (2,), True),        (1, 64, 65)),             # S = 17: one thread per table row; three tiles
}


@functools.lru_cache(maxsize=None)
def edge_state(name):
    shape, sizes = EDGE_SHAPES[name]
    return _state_of(name, make_workload(f"srcdraw_{name}", shape=shape)), sizes


@functools.lru_cache(maxsize=None)
def single_component_state():
    """C = 1: clusters alone, every object in one (an object in none would have no weight row), the cdf of every row is [1]."""
    wl = make_workload("srcdraw_c1", shape=(40, 17, 4, 3, (), True))
    N, F, S = wl.features.shape
    K = 3
    clusters = np.arange(N)[None, :] % K == np.arange(K)[:, None]
    na = ~wl.features.any(-1)
    source = (~na)[..., None].copy()
    return State(name="c1", features=wl.features.copy(), groups=[clusters], conc=[wl.concentration[0].copy()],
                 weights=np.ones((F, 1), dtype=F32), source=source, unif=wl.states_per_feature.astype(np.float64))


def subsets(N, size, seed):
    """(ascending, shuffled) object lists of `size` objects."""
    rng = np.random.default_rng(seed)
    asc = np.sort(rng.choice(N, size=size, replace=False)).astype(np.int32)
    return asc, asc[rng.permutation(size)]
