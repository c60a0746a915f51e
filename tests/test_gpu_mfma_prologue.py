"""The matrix-pipe mixture kernel's work AROUND its passes (k_mixture_tuple_mfma): the A image built by byte permute (blocks of up
to 8 tuples) or by byte compares (wider blocks), the pass's first k-block written without a zeroed accumulator, the X-fragment
ring, the shared-operand descriptors asked for ahead of phase 0.  These can only go wrong at edges, so the shapes are small and
chosen for the edges:

* N around a k-block boundary (64 objects; a lane half holds 32): the last id word of a lane half partly or wholly beyond N, and
  at N <= 64 the peeled first k-block is the only one with data (KBp is padded to a multiple of 4: the others are all-zero).
* Tuple counts 1, 2, 7, 8 (byte-permute build; 16 and 4 slots per block) and 9 (first wide form: byte compares).  A slot's tuples
  are numbered densely in order of first appearance (derive_tuples), so "tuple 0 is empty" and "everyone in the last tuple" cannot
  be written into the id array itself; the cases put every object of slot 1 into the LAST cluster (its ids are all 0 while the
  launch's other tuples stay empty for it) and leave cluster 0 of slot 2 empty (its id 0 is another cluster's tuple).
* Batch sizes 1, 15, 16, 17, 33 through a slot LIST that is not contiguous (the batched step's candidate slots): blocks with
  absent slots (filler ids, a descriptor thread whose slot is -1).
* 2 * 16 * 32 + 5 columns on 8 waves with one column split: two full passes and a third whose only tile is partly empty; the other
  waves and tile 33 read the zero tile.
* The same launch twice: equal as uint64.

Every case forces the matrix-pipe form, compares with the oracle at 1e-10 like the shape tests, and with the vector-pipe form of the
same table (k_mixture_tuple64 / k_mixture_combo) at 1e-12.  The two forms cannot be expected to agree bit for bit at any shape
with more than one observation: the vector-pipe form builds the table of logs in LDS with its own 128-interval table log (1.5 ulp)
and adds one gathered value per OBSERVATION, object by object; this kernel takes its 1024-interval log of the mantissa per table
ENTRY, multiplies it by the entry's count and sums the binary exponents apart as integers -- different roundings of different
terms.  The bit-for-bit checks are therefore the repeated launch and, for the shared-operand epilogue,
tests/test_gpu_shared_epilogue.py (per-entry against shared form).  test_case_oracles_cpu checks without a GPU that every case's
oracle value is finite and within 1e-12 of an extended-precision evaluation of the same expression."""
import functools

import numpy as np
import pytest

from oracle import sbayes_oracle as orc
from sbayes_amd.engine import MIXTURE_PACKED_TUPLE, MIXTURE_PACKED_TUPLE_MFMA, Engine

N_SWEEP = [1, 31, 32, 33, 63, 64, 65, 127, 129]
KT_SWEEP = [1, 2, 7, 8, 9]
B_SWEEP = [1, 15, 16, 17, 33]
MULTI_PASS = dict(N=200, F=343, S=3, KT=3, B=17)            # F * S = 1029 = 2 * 16 * 32 + 5 columns


@functools.lru_cache(maxsize=None)
def make_case(N, F, S, KT, B, seed):
    """B states over one feature block with exactly KT group tuples in the launch (C = 2: KT - 1 clusters + "no cluster" under a
    universal confounder; KT = 1: one cluster that holds everyone).  -> (feats, n_groups, conc, states, want): states[b] = (groups,
    weights, source), want[b] = the oracle's value.  Computed once per case and shared (read-only)."""
    rng = np.random.default_rng(seed)
    K = max(KT - 1, 1)
    n_groups = [K, 1]
    x = rng.integers(0, S, size=(N, F))
    na = rng.random((N, F)) < 0.05
    feats = np.zeros((N, F, S), dtype=bool)
    nn, ff = np.nonzero(~na)
    feats[nn, ff, x[nn, ff]] = True
    conf = np.ones((1, N), dtype=bool)
    conc = [rng.choice([0.5, 1.0, 2.0], size=(F, S)), rng.choice([0.5, 1.0, 2.0], size=(1, F, S))]
    states, want = [], []
    for b in range(B):
        a = rng.integers(0, KT, size=N) if KT > 1 else np.zeros(N, dtype=np.int64)      # K = KT - 1: no cluster
        if b == 0 and N >= KT:
            a[rng.permutation(N)[:KT]] = np.arange(KT)          # slot 0 has every tuple
        if b == 1:
            a[:] = K - 1                                          # everyone in the last cluster
        if b == 2 and KT > 1:
            a[a == 0] = K if K == 1 else 1                        # cluster 0 empty
        groups = [np.stack([a == k for k in range(K)]), conf]
        weights = rng.dirichlet(np.ones(2), size=F).astype(np.float32)
        hc = orc.has_components(groups)
        source = np.eye(2, dtype=bool)[np.argmax(rng.random((N, F, 2)) * hc[:, None, :], axis=-1)]
        source[na] = False
        counts = orc.recalculate_feature_counts(feats, groups, source)
        states.append((groups, weights, source))
        want.append(orc.mixture_loglik(feats, na, groups, counts, conc, weights))
    feats.setflags(write=False)
    return feats, n_groups, conc, states, np.array(want)


def all_cases():
    cases = [(N, 3, 4, 3, 5, 100 + N) for N in N_SWEEP]
    cases += [(100, 7, 3, KT, 6, 200 + KT) for KT in KT_SWEEP]
    cases += [(70, 5, 3, 4, B, 300 + B) for B in B_SWEEP]
    m = MULTI_PASS
    cases.append((m["N"], m["F"], m["S"], m["KT"], m["B"], 400))
    return cases


def test_case_oracles_cpu():
    """Every case's oracle value is finite and within 1e-12 of the same expression evaluated in extended precision (the kernel
    is held to 1e-10)."""
    for (N, F, S, KT, B, seed) in all_cases():
        feats, n_groups, conc, states, want = make_case(N, F, S, KT, B, seed)
        assert want.shape == (B,) and np.all(np.isfinite(want)) and np.all(want < 0), (N, F, S, KT, B)
        na = ~feats.any(-1)
        for b in sorted({0, min(1, B - 1), min(2, B - 1), B - 1}):
            groups, weights, source = states[b]
            counts = orc.recalculate_feature_counts(feats, groups, source)
            lh = orc.likelihood_per_component(feats, na, groups, counts, conc)
            w = orc.normalize_weights(weights, orc.has_components(groups))
            obs = (w.astype(np.longdouble) * lh.astype(np.longdouble)).sum(-1)
            ref = np.log(obs)[~na].sum()
            assert abs(want[b] - float(ref)) <= 1e-12 * abs(float(ref)), (N, F, S, KT, B, b, want[b], float(ref))
        cl0 = states[0][0][0]                                     # slot 0 holds every tuple of the launch
        labels = np.where(cl0.any(0), cl0.argmax(0), cl0.shape[0])
        if N >= KT:
            assert len(np.unique(labels)) == KT, (KT, np.unique(labels))


def _load(eng, conc, states, slots):
    for c in range(2):
        eng.set_concentration(c, conc[c])
    for slot, (groups, weights, source) in zip(slots, states):
        eng.load_state(int(slot), groups, weights, source=source)
        for c in range(2):
            eng.update_probs(int(slot), c)


def _check_batch(case, slots_per_block, monkeypatch, expect=None):
    """The case through mixture_loglik_batch in the matrix-pipe form: oracle, repeat launch, the vector-pipe form."""
    if slots_per_block == 16:
        monkeypatch.setenv("SBE_MFMA_SMALL_SL4", "0")            # (read when the engine is created)
    else:
        monkeypatch.delenv("SBE_MFMA_SMALL_SL4", raising=False)
    feats, n_groups, conc, states, want = make_case(*case)
    B = len(states)
    with Engine(np.array(feats), n_groups, n_slots=B) as eng:
        _load(eng, conc, states, range(B))
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        got = eng.mixture_loglik_batch(0, B)
        name = eng.last_mixture_kernel()
        assert "k_mixture_tuple_mfma<" in name, name
        if expect is not None:
            assert expect in name, name
        again = eng.mixture_loglik_batch(0, B)
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE)
        other = eng.mixture_loglik_batch(0, B)
        assert "k_mixture_tuple_mfma" not in eng.last_mixture_kernel()
    print(case, name, "max rel.err vs oracle", np.max(np.abs(got - want) / np.abs(want)))
    np.testing.assert_allclose(got, want, rtol=1e-10)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    np.testing.assert_allclose(other, got, rtol=1e-12)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("slots_per_block", [16, 4])
@pytest.mark.parametrize("N", N_SWEEP)
def test_objects_around_a_k_block_boundary(N, slots_per_block, monkeypatch):
    # (three tuples = two M tiles of 16 slots: small launches then take four slots per block unless the switch says otherwise;
    #  a single object has a single tuple, and one M tile stays with 16 slots)
    _check_batch((N, 3, 4, 3, 5, 100 + N), slots_per_block, monkeypatch, expect=f"{slots_per_block if N > 1 else 16} slots")


@pytest.mark.gpu
@pytest.mark.parametrize("slots_per_block", [16, 4])
@pytest.mark.parametrize("KT", KT_SWEEP)
def test_tuple_counts_across_the_eight_tuple_limit(KT, slots_per_block, monkeypatch):
    """KT <= 8: 16 slots x ceil(KT / 2) M tiles or 4 slots x 1 M tile, ids looked up by byte permute; KT = 9: the first wide form
    (4 slots x 2 M tiles: 16 tuples per block, ids compared byte by byte) whatever the switch says."""
    if KT <= 8:
        # (four slots per block are taken where they save M tiles: not at one M tile of 16 slots)
        expect = f"16 slots x M tiles {(KT + 1) // 2}" if slots_per_block == 16 or KT <= 2 else "4 slots x M tiles 1"
    else:
        expect = "4 slots x M tiles 2"
    _check_batch((100, 7, 3, KT, 6, 200 + KT), slots_per_block, monkeypatch, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize("slots_per_block", [16, 4])
@pytest.mark.parametrize("B", B_SWEEP)
def test_batch_sizes_through_a_slot_list(B, slots_per_block, monkeypatch):
    """The batched step evaluates its candidate slots from a list: B chains with an empty proposal, candidates scattered over the
    engine's slots in no order.  Every chain's mixture value is its state's."""
    if slots_per_block == 16:
        monkeypatch.setenv("SBE_MFMA_SMALL_SL4", "0")
    else:
        monkeypatch.delenv("SBE_MFMA_SMALL_SL4", raising=False)
    feats, n_groups, conc, states, want = make_case(70, 5, 3, 4, B, 300 + B)
    rng = np.random.default_rng(B)
    perm = rng.permutation(B)
    cur = (3 * perm).astype(np.int32)                              # chain i: state i in slot 3 perm[i], candidate two slots on
    cand = (cur + 2).astype(np.int32)
    with Engine(np.array(feats), n_groups, n_slots=3 * B) as eng:
        _load(eng, conc, states, cur)
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE_MFMA)
        _glh, mix, _changed = eng.step_batch(cur, cand)
        name = eng.last_mixture_kernel()
        assert "k_mixture_tuple_mfma<" in name and f"{slots_per_block} slots" in name, name
        _glh, again, _changed = eng.step_batch(cur, cand)
        eng.set_option(kernel=MIXTURE_PACKED_TUPLE)
        singles = np.array([eng.mixture_loglik(int(s)) for s in cand])
    print(B, name, "max rel.err vs oracle", np.max(np.abs(mix - want) / np.abs(want)))
    np.testing.assert_allclose(mix, want, rtol=1e-10)
    assert np.array_equal(mix.view(np.uint64), again.view(np.uint64))
    np.testing.assert_allclose(singles, mix, rtol=1e-12)


@pytest.mark.gpu
def test_three_passes_with_a_partly_empty_last_tile(monkeypatch):
    """1029 columns = 33 column tiles walked by ONE block per 16 slots (a single column split): 8 waves x 2 tiles per pass, so two
    full passes and a third in which wave 0 holds tile 32 (5 columns) beside the zero tile and the other waves have nothing.  The
    default geometry (several column splits) gives the same values to rounding."""
    m = MULTI_PASS
    case = (m["N"], m["F"], m["S"], m["KT"], m["B"], 400)
    monkeypatch.setenv("SBE_MFMA_SPLIT", "1")
    one_split = _check_batch(case, 16, monkeypatch, expect="16 slots x M tiles 2")
    monkeypatch.delenv("SBE_MFMA_SPLIT")
    np.testing.assert_allclose(_check_batch(case, 16, monkeypatch), one_split, rtol=1e-12)


@pytest.mark.gpu
def test_repeated_launch_is_bit_identical(monkeypatch):
    """One case (N = 65: a second k-block with one object; 16 slots per block, 5 of them present) launched twice in two engines:
    the four results are equal as uint64."""
    case = (65, 3, 4, 3, 5, 165)
    first = _check_batch(case, 16, monkeypatch)
    second = _check_batch(case, 16, monkeypatch)
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
