"""configs[1] as three device-generated batches on one engine; prints, per batch, the time and rb2_hip_steady_stats: the round the device first
reported a round of fused tiles at, the round the host used it from, and the share of the batch's dense rounds that ran the k_advance without the
group search / no k_prep<AE> ("the steady round").  RB2_STEADY_AHEAD=0: without the run-ahead bound."""
import os, sys, time
sys.path.insert(0, os.getcwd())
from ropebwt2_amd import HipBwt
n, L = 100_000_000, 101
per = (4 << 30) // (L + 1)       # reads per -m4g batch (approx.)
dev = HipBwt(1)
first, prev, prev_lean = 0, (0, 0), 0
while first < n:
    cnt = min(per, n - first)
    p = dev.dev_alloc(cnt * (L + 1))
    dev.synth_reads(p, first, cnt, L, seed=42)
    dev.sync()
    t0 = time.time()
    dev.insert_multi_dev(p, cnt * (L + 1))
    dev.sync()
    st = dev.steady_stats()
    ln = dev.lean_stats()
    a, s = st["advance_single"] - prev[0], st["prep_skipped"] - prev[1]
    prev = (st["advance_single"], st["prep_skipped"])
    print("batch", first, cnt, "%.3f s" % (time.time() - t0), "reported_at", st["reported_at"], "used_from", st["used_from"],
          "rounds %d: %d single k_advance (%.0f %%), %d without k_prep, %d lean (stage %d)" % (L + 1, a, 100.0 * a / (L + 1), s, ln["rounds"] - prev_lean, ln["stage"]), flush=True)
    prev_lean = ln["rounds"]
    dev.dev_free(p)
    first += cnt
