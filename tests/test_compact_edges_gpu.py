"""k_merge's window formats (csrc/rb2_merge.h) at their edges, round by round: inputs that hold exactly 63, 64, 127, 128 ... exceptions
per window and are read back at every offset BY CONSTRUCTION (compact_edge_jobs.py), ropes and matrix bit-exact against the oracle after
every batch, and the windows the engine wrote in each format EQUAL to what the per-round model (bcr_rounds_ref.py) says it must have
written -- an off-by-one in a threshold is caught in either direction, the harmless one (a 63-exception window written with two lines:
the BWT is still right) included.  What the inputs reach is checked on the model, before the GPU is touched (and in
test_bcr_rounds_ref.py without one).
"""
import numpy as np
import pytest

import bcr_rounds_ref as R
import compact_edge_jobs as J
import helpers as H
from test_compact_gpu import Env, _run, _same

pytestmark = pytest.mark.gpu

KEYS = ["plain", "compact0", "compact1", "compact2", "compact_rounds"]
_model = {}


def model(name, compact=True):
    """the model's sums over a job, and the coverage its rounds reach"""
    if (name, compact) not in _model:
        m, cov = R.RoundsModel(compact), R.Coverage()
        for buf in J.job(name):
            m.insert_multi(buf, cov.add)
        _model[name, compact] = (m.stats, cov)
    return _model[name, compact]


def _covered():
    """the condition on the inputs: over the compact rounds of the designed jobs the model reports every case (bcr_rounds_ref.required_cases)"""
    seen = set()
    for name in J.JOBS:
        seen |= model(name)[1].seen
    missing = [c for c in R.required_cases() if c not in seen]
    assert not missing, "the designed inputs do not reach: %s" % missing


@pytest.mark.parametrize("name", list(J.JOBS))
def test_windows_per_format_equal_the_model(hip, name):
    _covered()
    want = model(name)[0]
    st = _run(hip, 0, J.job(name))                                  # ropes and matrix against the oracle after every batch
    print("engine", st, "model", want)
    assert st["counted"]
    # the engine counts one window per WPL leaves of every piece that holds a symbol, in every round of every batch (k_setup: nwin per piece
    # = ceil(ceil(n / LEAF) / WPL), none for an empty piece; k_merge: gw < wf0[NR]) -- the model's windows, no padding
    assert {k: st[k] for k in KEYS} == want


@pytest.mark.parametrize("name", list(J.JOBS))
def test_compact_off_is_the_same_index(hip, name):
    """RB2_COMPACT=0: the same ropes (against the oracle and, by their device checksums, against the compact run), plain windows only --
    as many as the model has windows"""
    _covered()
    hs = []
    for off in (False, True):
        with Env(RB2_COMPACT_STATS=1, RB2_SPARSE_LAMBDA=0, **({"RB2_COMPACT": 0} if off else {})):
            dev, o = hip.HipBwt(0), H.Oracle(0)
            for buf in J.job(name):
                o.insert_multi(buf)
                dev.insert_multi(buf)
                _same(dev, o)
            hs.append(dev.rope_hashes())
            st = dev.window_stats()
            dev.close()
    assert hs[0] == hs[1]
    print("engine", st, "model", model(name, False)[0])
    assert {k: st[k] for k in KEYS} == model(name, False)[0]
    assert st["compact_rounds"] == 0 and st["compact0"] + st["compact1"] + st["compact2"] == 0


def test_two_ranks_write_the_model_s_windows(hip):
    """pieces are the unit of ownership, so the windows of two ranks together are the model's windows; in input order every rank knows
    from the start that all intervals are empty (B.known_ae), so each of them allows compact windows in the same rounds as one engine"""
    from ropebwt2_amd.hipbwt import MultiBwt
    _covered()
    want = model("designed")[0]
    with Env(RB2_COMPACT_STATS=1, RB2_SPARSE_LAMBDA=0):
        m, o = MultiBwt(0, [0, 0], "peer"), H.Oracle(0)
        for buf in J.job("designed"):
            o.insert_multi(buf)
            m.insert_multi(buf)
            assert np.array_equal(m.counts(), o.counts())
            for b in range(6):
                assert np.array_equal(m.rope(b), o.rope(b)), "rope %d" % b
        ws = [m.engine(k).window_stats() for k in range(2)]
        m.close()
    print("ranks", ws, "model", want)
    assert all(w["counted"] for w in ws)
    assert {k: sum(w[k] for w in ws) for k in KEYS[:4]} == {k: want[k] for k in KEYS[:4]}
    assert [w["compact_rounds"] for w in ws] == [want["compact_rounds"]] * 2
