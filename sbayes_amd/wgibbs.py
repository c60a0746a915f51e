"""The Gibbs weights operator's step on the device (include/sbe_wgibbs.h).

sBayes' GibbsSampleWeights._propose (sbayes/sampling/operators.py:597-676) picks two mixture components, draws a new split
of their joint weight per feature from a beta distribution built on source counts, and accepts or rejects every
feature's new weight row on its own.  Under patch.install(operators=True) its body still runs as NumPy / SciPy around
the one piece with a device form (source_lh_by_feature): an [N, F, C] boolean sum, two Python loops of
scipy.stats.dirichlet log-pdfs over the features, a frozen scipy.stats.beta with two logpdf calls, update_weights twice.
Everything of it that draws no random number is two engine calls on the slot the sample is bound to:

    pair_counts(eng, slot, i1, i2)                                  # int32 [F, 2]
    step(eng, slot, i1, i2, a2, u, alpha, beta_ab, prior_temperature)   # (weights float32 [F, C], accept bool [F], log_p)
    gibbs_sample_weights(op, sample, eng)                           # the whole _propose: draws on the host, the rest here
    patch.install(gibbs_weights=True)                               # swaps GibbsSampleWeights._propose

Numerical contract (tests/_wgibbs_oracle.py restates it in NumPy).  The proposed weights are the
reference's float32 values bit for bit.  The Metropolis log ratio is taken in float64 as a sum of differences of logs:
ln B(alpha) of the Dirichlet prior and betaln of the beta proposal are the same on both sides and never computed.  The
reference adds N float32 logs per feature in float32, twice; its log ratio differs from the float64 one by up to
(N + 1) 2^-24 times the sum of the |log| terms, so a decision whose uniform lies that close to p can differ.  The three
random streams (`random`, `np.random`, the reference's module-level `RNG`) are consumed in the reference's order and
amounts: i1, i2 = random.sample(range(C), 2); a2 = np.random.beta(1 + c2, 1 + c1, size=F) -- what
scipy.stats.beta(...).rvs() draws, bit for bit; u = RNG.random(F, dtype=float32).

The slot is left untouched: the accepted weights go into the sample, and the next bind uploads their F * C floats."""
from __future__ import annotations

import ctypes as ct
import importlib
import math
import random

import numpy as np

from . import _handle

ABI_VERSION = 1                          # SBE_WGIBBS_ABI_VERSION of include/sbe_wgibbs.h
FEATURE_TILE = 16                        # SBE_WGIBBS_FEATURE_TILE
COVERED_PRIORS = ("uniform", "jeffreys", "BBS", "symmetric_dirichlet")

# name -> (restype, argtypes); mirrors include/sbe_wgibbs.h one to one (the engine's own table, _lib.PROTOTYPES, is not extended)
PROTOTYPES = {
    "sbe_wgibbs_abi_version": (ct.c_int, []),
    "sbe_wgibbs_pair_counts": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p]),
    "sbe_wgibbs_step": (ct.c_int, [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                   ct.c_double, ct.c_void_p, ct.c_void_p, ct.c_void_p]),
}


def load():
    """The engine library with the prototypes of include/sbe_wgibbs.h attached."""
    return _handle.bind("sbe_wgibbs", PROTOTYPES, ABI_VERSION)


# ---- validation (host side, before any library call) -----------------------------------------------------------
def _check_pair(eng, slot, i1, i2):
    slot, i1, i2 = int(slot), int(i1), int(i2)
    if not 0 <= slot < eng.n_slots:
        raise ValueError(f"slot {slot} out of range [0, {eng.n_slots})")
    c = eng.n_components
    if not (0 <= i1 < c and 0 <= i2 < c) or i1 == i2:
        raise ValueError(f"components ({i1}, {i2}): two different indices in [0, {c}) are needed")
    return slot, i1, i2


def _array(a, dtype, shape, name):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
    return a


def pair_counts(eng, slot, i1, i2):
    """int32 [F, 2]: per feature, the objects of `slot` whose has_components pattern has both components and whose source
    is i1 (column 0) / i2 (column 1): np.sum(source[has_both], axis=0)[:, [i1, i2]] of the reference."""
    slot, i1, i2 = _check_pair(eng, slot, i1, i2)
    lib = load()
    out = np.empty((eng.n_features, 2), dtype=np.int32)
    eng._check(lib.sbe_wgibbs_pair_counts(eng._h, slot, i1, i2, eng._o(out)))
    return out


def step(eng, slot, i1, i2, a2, u, alpha, beta_ab, prior_temperature, want_log_p=True):
    """The step after the draws on the state of `slot`: (weights float32 [F, C], accept bool [F], log_p float64 [F] or
    None).  a2 float64 [F], u float32 [F], alpha float64 [F, C], beta_ab float64 [F, 2] = (A, B) of the beta proposal."""
    slot, i1, i2 = _check_pair(eng, slot, i1, i2)
    f, c = eng.n_features, eng.n_components
    t = float(prior_temperature)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"prior_temperature must be positive and finite, got {prior_temperature!r}")
    a2 = _array(a2, np.float64, (f,), "a2")
    u = _array(u, np.float32, (f,), "u")
    alpha = _array(alpha, np.float64, (f, c), "alpha")
    beta_ab = _array(beta_ab, np.float64, (f, 2), "beta_ab")
    lib = load()
    w_out = np.empty((f, c), dtype=np.float32)
    accept = np.empty(f, dtype=np.uint8)
    log_p = np.empty(f, dtype=np.float64) if want_log_p else None
    eng._check(lib.sbe_wgibbs_step(eng._h, slot, i1, i2, eng._i(a2), eng._i(u), eng._i(alpha), eng._i(beta_ab), t, eng._o(w_out),
                                   eng._o(accept), eng._o(log_p) if want_log_p else None))
    return w_out, accept.view(np.bool_), log_p


# ---- the operator ----------------------------------------------------------------------------------------------
def covered(op, sample):
    """Does the device form take this operator's proposal?  The weights prior is one of COVERED_PRIORS (a Dirichlet with a
    fixed concentration per feature) and there are two components to pick."""
    prior_w = getattr(getattr(op.model, "prior", None), "prior_weights", None)
    kind = getattr(getattr(prior_w, "prior_type", None), "value", None)
    return kind in COVERED_PRIORS and int(sample.n_components) >= 2


def engine_for(op, sample):
    """The live engine that holds this operator's observations, or None: the conditions of the device form of
    source_lh_by_feature (patch.py) -- only the layout computation and the lookup may decline."""
    from . import registry
    try:
        na = op.model.likelihood.na_features
        layout = [sample.clusters.value.shape[0]] + [c.group_assignment.shape[0] for c in sample.confounders.values()]
        return registry.engine_for_observations(na, int(sample.n_components), layout)
    except (ValueError, AttributeError):
        return None


def _alpha(prior_w, shape):
    """float64 [F, C] of the prior's concentration list, kept on the prior object (it is fixed for these prior types)."""
    cached = prior_w.__dict__.get("_sbayes_amd_alpha")
    if cached is None or cached[0] is not prior_w.concentration:
        cached = (prior_w.concentration, np.ascontiguousarray(prior_w.concentration, dtype=np.float64))
        prior_w.__dict__["_sbayes_amd_alpha"] = cached
    if cached[1].shape != shape:
        raise ValueError(f"the weights prior's concentration has shape {cached[1].shape}, the weights {shape}")
    return cached[1]


def gibbs_sample_weights(op, sample, eng):
    """GibbsSampleWeights._propose (operators.py:597-676) with everything after the random draws on the device.  Leaves the
    sample as the reference does: the new weights, sample.weights.version advanced twice, op.last_accept_rate set."""
    from .binding import _bind_slot
    rng = importlib.import_module(type(op).__module__).RNG     # the reference's module-level generator (sbayes/util.py:36)
    prior_w = op.model.prior.prior_weights
    t = op.prior_temperature
    n_features, n_components = sample.weights.value.shape
    _bind_slot(eng, None, sample, 0, with_source=True)
    i1, i2 = random.sample(range(sample.n_components), 2)
    counts = pair_counts(eng, 0, i1, i2)
    c = (counts + prior_w.concentration_array[:, [i1, i2]]) / t
    beta_ab = np.empty((n_features, 2), dtype=np.float64)
    beta_ab[:, 0] = 1 + c[:, 1]
    beta_ab[:, 1] = 1 + c[:, 0]
    a2 = np.random.beta(beta_ab[:, 0], beta_ab[:, 1], size=n_features)
    u = rng.random(n_features, dtype=np.float32)
    w_out, accept, _ = step(eng, 0, i1, i2, a2, u, _alpha(prior_w, (n_features, n_components)), beta_ab, t, want_log_p=False)
    sample.weights.set_value(w_out)          # (twice, as the reference: the proposal, then the accepted rows)
    sample.weights.set_value(w_out)
    assert ~np.any(np.isnan(sample.weights.value))
    op.last_accept_rate = np.mean(accept)
    return sample, op.Q_GIBBS, op.Q_BACK_GIBBS
