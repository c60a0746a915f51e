"""Test double for the two calls of sbayes_amd.wgibbs (pair_counts, step) on the oracle-backed FakeEngine
(tests/_fake_engine.py, not edited): the float64 restatement of tests/_wgibbs_oracle.py evaluated on the double's slot
state -- TEST INFRASTRUCTURE.  `install(monkeypatch)` puts both in place of the library calls and returns the list that
collects one record per step (the draws, the restatement's log_p and terms)."""
import numpy as np

from oracle import sbayes_oracle as orc
from tests import _wgibbs_oracle as worc


def slot_state(eng, slot):
    s = eng.slots[slot]
    groups = [s["groups"][c] for c in range(len(s["groups"]))]
    patterns, pid, src = worc.state_of(orc.has_components(groups), s["source"], eng.na_values())
    return np.asarray(s["weights"], dtype=np.float32), patterns, pid, src, eng.na_values()


def pair_counts(eng, slot, i1, i2):
    eng.calls.append(("wgibbs_pair_counts", int(i1), int(i2)))
    _w, patterns, pid, src, na = slot_state(eng, slot)
    return worc.pair_counts(patterns, pid, src, na, i1, i2).astype(np.int32)


def make_step(records):
    def step(eng, slot, i1, i2, a2, u, alpha, beta_ab, prior_temperature, want_log_p=True):
        eng.calls.append(("wgibbs_step", int(i1), int(i2)))
        w, patterns, pid, src, na = slot_state(eng, slot)
        w_out, accept, terms, w_new = worc.step(w, patterns, pid, src, na, i1, i2, a2, u, alpha, beta_ab, prior_temperature)
        records.append(dict(i12=(int(i1), int(i2)), a2=np.array(a2), u=np.array(u), beta_ab=np.array(beta_ab), w=w.copy(),
                            w_new=w_new, accept=accept, terms=terms, prior_temperature=float(prior_temperature)))
        return w_out, accept, terms["log_p"] if want_log_p else None
    return step


def install(monkeypatch):
    from sbayes_amd import wgibbs
    records = []
    monkeypatch.setattr(wgibbs, "pair_counts", pair_counts)
    monkeypatch.setattr(wgibbs, "step", make_step(records))
    return records
