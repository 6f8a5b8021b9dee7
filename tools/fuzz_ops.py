#!/usr/bin/env python3
"""Randomised sequence run on the GPU box: scripts of mixed operations on one handle (inserts from host, prefetched, registered and device
buffers, delete, merge, the loaders, reset, the sampled suffix array, reserve) against the CPU model of tests/op_sequences.py, compared
exactly after every step; the seed picks the sorting order and the layout profile.  Test infrastructure (uses oracle/ through tests/helpers.py);
stops at the first mismatch and prints the script as data, with the step.
usage: fuzz_ops.py [seconds=300] [first_seed=1]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H
from ropebwt2_amd import HipBwt, build_all
build_all(); H.build_oracle()
import op_sequences as S

ENVS = {"default": {}, "sparse": {"RB2_SPARSE_LAMBDA": "1e18", "RB2_SPARSE_MAXPEN": "0"}, "dense": {"RB2_SPARSE_LAMBDA": "0"}}

def maker(so, env):
    def make():                                                    # (the environment is read at create)
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return HipBwt(so)
        finally:
            for k, v in old.items():
                if v is None: os.environ.pop(k, None)
                else: os.environ[k] = v
    return make

def one(seed):
    so, profile = seed % 3, S.PROFILES[seed // 3 % 3]
    try:
        S.run(S.script(seed, so, profile), maker(so, ENVS[profile]))
    except S.StepFailed as e:
        return "seed %d, so %d, profile %s\n%s" % (seed, so, profile, e)
    return None

def main():
    secs = float(sys.argv[1]) if len(sys.argv) > 1 else 300.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    t0, n = time.time(), 0
    while time.time() - t0 < secs:
        r = one(seed)
        if r is not None:
            print(r); print("MISMATCH after %d scripts" % n); sys.exit(1)
        seed += 1; n += 1
    print("fuzz_ops: %d scripts (seeds %d..%d) in %.0f s, all equal to the model" % (n, seed - n, seed - 1, time.time() - t0))

if __name__ == "__main__":
    main()
