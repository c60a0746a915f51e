"""The seeded cases of the pairwise posterior predictive check, shared by tests/test_pairppc_oracle_cpu.py (which proves under
the oracle alone that every case holds what it claims) and tests/test_gpu_pairppc.py (device against oracle).  A plain helper
module: it holds no test.

A case is (x uint8 [N, F], n_states int32 [F], y uint8 [T, N, F]) with T = 7 replicates (4 in the two wide cases), all read-only, and the oracle's result,
computed once.  The data follow a latent state per object (so that pairs depend on each other), state counts are ragged within
one data set, F fills more than one 32-column tile and is no multiple of the features per tile edge (off-diagonal tile pairs and
a ragged last tile), N lies at the edges of the 256 objects the codes are padded to.  The replicates keep the data's missingness:

  replicate 0   the data itself: every valid pair ties (n_equal);
  replicate 1   the data with the two states of binary feature SWAPPED exchanged: the same tables with two rows exchanged;
  replicate 2   the data with feature CONSTANT set to state 0 wherever observed: its pairs are degenerate, s = 0;
  replicates 3 ..     every column permuted on its own among its observed objects: independent features with the data's margins."""
from __future__ import annotations

import functools

import numpy as np

from tests import _pairppc_oracle as orc

NA = orc.NA
T = 7
SAME, SWAP, DEGENERATE = 0, 1, 2
SWAPPED, CONSTANT = 1, 0                 # the features replicates 1 and 2 change

# name -> (seed, S_pad, F, N, NA rate, feature observed nowhere or None, feature with one state on the data or None)
CASES = {
    "s2": (11, 2, 33, 257, 0.3, None, None),
    "s4": (12, 4, 17, 255, 0.0, None, None),
    "s8": (13, 8, 9, 256, 0.3, 2, 3),
    "s16": (14, 16, 5, 257, 0.0, None, None),
    "s32": (15, 32, 3, 255, 0.3, None, None),
    "one_object": (16, 4, 17, 1, 0.0, None, None),
    # the two sides of the 8192 tile pairs below which the unit itself picks the spread form (csrc/sbe_pairppc.hip; a tile edge holds two features at S_pad = 16): 127 tiles make
    # 8128 pairs, 128 tiles 8256; four replicates each
    "below_spread": (17, 16, 253, 33, 0.0, None, None),
    "at_spread": (18, 16, 255, 33, 0.0, None, None),
}
WIDE = ("below_spread", "at_spread")     # (too many pairs for a loop in Python)
T_WIDE = 4


def sub_of(s_pad):
    """Features per tile edge at S_pad."""
    return 32 // s_pad


def _build(name):
    seed, s_pad, f, n, na_rate, nowhere, one_state = CASES[name]
    rng = np.random.default_rng(seed)
    ns = rng.integers(2, s_pad + 1, f).astype(np.int32)
    ns[0], ns[SWAPPED] = s_pad, 2
    if s_pad == 2:
        ns[-1] = 1                                            # ragged at S_pad = 2: a feature of one state
    if s_pad == 32:
        ns[-1] = 17                                           # (a tile holds one feature there: the last tile is partial by its states)
    theta = np.linspace(0.2, 0.9, f)[rng.permutation(f)]
    latent = rng.integers(0, s_pad, n)
    x = np.empty((n, f), dtype=np.uint8)
    for k in range(f):
        follow = rng.random(n) < theta[k]
        x[:, k] = np.where(follow, latent % ns[k], rng.integers(0, ns[k], n))
    if one_state is not None:
        x[:, one_state] = 1                                   # (n_states stays: the replicates may show the other states)
    x[rng.random((n, f)) < na_rate] = NA
    if nowhere is not None:
        x[:, nowhere] = NA
    t_n = T_WIDE if name in WIDE else T
    y = np.repeat(x[None], t_n, axis=0)
    y[SWAP, :, SWAPPED] = np.where(x[:, SWAPPED] == NA, NA, 1 - np.minimum(x[:, SWAPPED], 1))
    y[DEGENERATE, :, CONSTANT] = np.where(x[:, CONSTANT] == NA, NA, 0)
    for t in range(3, t_n):
        for k in range(f):
            at = np.nonzero(x[:, k] != NA)[0]
            y[t, at, k] = x[rng.permutation(at), k]
    if one_state is not None:                                 # the replicates of that feature do vary
        at = np.nonzero(x[:, one_state] != NA)[0]
        for t in range(3, t_n):
            y[t, at, one_state] = rng.integers(0, ns[one_state], at.size)
    return x, ns, y


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, n_states, y, the oracle's result) of the case."""
    x, ns, y = _build(name)
    for a in (x, ns, y):
        a.setflags(write=False)
    return x, ns, y, orc.check(x, ns, y)


def hand():
    """Six objects, two binary features and one ternary, worked by hand.  Features 0 and 1 agree on every object
    (table [[3, 0], [0, 3]]: E = 1.5 everywhere, Yates leaves |O - E| - 1/2 = 1, statistic 4 * 1 / 1.5 = 8/3); feature 2 runs
    0, 1, 2, 0, 1, 2 against 0, 0, 0, 1, 1, 1 (table [[1, 1, 1], [1, 1, 1]]: E = O, statistic 0 at dof 2).
      replicate 0: the data -- every pair ties;
      replicate 1: feature 0 with its labels swapped -- the table of (0, 1) is [[0, 3], [3, 0]], the same statistic: a tie again;
      replicate 2: feature 1 = 0, 1, 0, 0, 1, 1 against feature 0 = 0, 0, 0, 1, 1, 1: table [[2, 1], [1, 2]], |O - E| = 1/2, Yates
                   removes all of it: statistic 0 < 8/3; against feature 2 = 0, 1, 2, 0, 1, 2: table [[2, 0, 1], [0, 2, 1]] at dof 2,
                   E = 1 everywhere, statistic 4 > 0.
    So pair (0, 1): n_greater 0, n_equal 2, n_less 1, p = 1/3; pair (0, 2): three ties, p = 1/2; pair (1, 2): n_greater 1,
    n_equal 2, p = 2/3, sum 4, sumsq 16."""
    x = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2], [1, 1, 0], [1, 1, 1], [1, 1, 2]], dtype=np.uint8)
    ns = np.array([2, 2, 3], dtype=np.int32)
    swapped = x.copy()
    swapped[:, 0] = 1 - x[:, 0]
    independent = x.copy()
    independent[:, 1] = [0, 1, 0, 0, 1, 1]
    return x, ns, np.stack([x, swapped, independent])
