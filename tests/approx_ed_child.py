"""child of tests/test_approx_ed_gpu.py, with a fatal handler installed that prints the message and leaves with status 7.  Every stage
first searches a small index (which must work: "approx_ed ok"), then calls both variants with n = 0 and the stage's bad parameters (which
must return: "empty ok"), then makes the one call that must be fatal; a call that returns prints "NOT FATAL".  The checks are made on
the host before anything is launched.
  ed-1 ed5 minocc0 steps0 recs0    a parameter of rb2_hip_approx_ed outside its range
  dev-ed5 dev-recs0                the same of rb2_hip_approx_ed_dev
  shard                            a rank of a sharded handle
usage: approx_ed_child.py STAGE"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
from ropebwt2_amd.hipbwt import HipBwt, MultiBwt, pack_patterns

#          max_ed, min_occ, max_steps, max_recs
STAGES = {"ed-1": (-1, 1, 100, 4), "ed5": (5, 1, 100, 4), "minocc0": (1, 0, 100, 4), "steps0": (1, 1, 0, 4), "recs0": (1, 1, 100, 0),
          "dev-ed5": (5, 1, 100, 4), "dev-recs0": (1, 1, 100, 0), "shard": (1, 1, 100, 4)}


def main():
    stage = sys.argv[1]
    max_ed, min_occ, max_steps, max_recs = STAGES[stage]
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    g = HipBwt(0)
    g.L.rb2_hip_set_fatal_handler(cb, None)
    reads = H.repetitive_reads(60, seed=9, max_len=30)
    g.insert_multi(H.encode_batch(reads, True, True))
    q = max(reads, key=len)
    stored, rec, cnt = g.approx_ed_raw([q], 1)
    assert cnt[0] >= 1 and stored == min(cnt[0], 64)
    print("approx_ed ok", flush=True)
    qry, off = pack_patterns([q])
    rec, cnt = np.zeros((1, 8, 4), np.int64), np.zeros(1, np.int64)
    args = (qry.ctypes.data, off.ctypes.data, max_ed, min_occ, max_steps, max_recs, rec.ctypes.data, cnt.ctypes.data)
    h = g.h
    if stage == "shard":
        m = MultiBwt(0, [0, 0])
        h = m.engine(0).h
    else:
        assert g.L.rb2_hip_approx_ed(h, 0, *args) == 0               # n <= 0 returns before the parameters are looked at
        g.L.rb2_hip_approx_ed_dev(h, 0, *args)
    print("empty ok", flush=True)
    if stage.startswith("dev-"):
        d = g.dev_alloc(4096)                                        # (the check comes before any pointer is used)
        g.L.rb2_hip_approx_ed_dev(h, 1, d, d, max_ed, min_occ, max_steps, max_recs, d, d)
    else:
        g.L.rb2_hip_approx_ed(h, 1, *args)
    print("NOT FATAL")


if __name__ == "__main__":
    main()
