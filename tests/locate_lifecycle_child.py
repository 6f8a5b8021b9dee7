"""child of tests/test_locate_gpu.py: the life of a sampled suffix array, with a fatal handler installed.  The handler prints the
message and leaves with status 7; a stage that must not be fatal ends with "STAGE OK" and status 0.  The stage "stream" is here because
torch has to open the device before the engine's library does when both live in one process, which a pytest session cannot promise.
usage: locate_lifecycle_child.py before | stale | life | stream"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import helpers as H
import locate_ref as LR
import query_ref as Q
from ropebwt2_amd.hipbwt import HipBwt

FORCED = dict(RB2_SPARSE_LAMBDA="1e18", RB2_SPARSE_MAXPEN="0")       # every batch in place: the sparse layout


def all_rows(g, fm):
    """every row through [x, x + 1) and through [0, N), against the model"""
    sid, pos, _ = LR.suffix_array(fm)
    want = np.stack([sid, pos], 1)
    x = np.arange(fm.N, dtype=np.int64)
    stored, hit, cnt = g.locate_raw(np.stack([x, x + 1], 1), 1)
    assert stored == fm.N and (cnt == 1).all() and np.array_equal(hit[:, 0], want)
    stored, hit, cnt = g.locate_raw([(0, fm.N)], fm.N)
    assert stored == fm.N and cnt.tolist() == [fm.N] and np.array_equal(hit[0], want)
    return want


def sparse_reads():
    """the reads of test_query_gpu.test_forced_sparse_layout: long reads with runs of N, then short repetitive ones"""
    rng = np.random.RandomState(3)
    reads = []
    for i in range(120):
        r = list(rng.randint(1, 5, size=int(rng.randint(1500, 2600))))
        for _ in range(int(rng.randint(0, 3))):
            at, n = int(rng.randint(0, len(r) - 1)), int(rng.randint(1, 300))
            r[at:at + n] = [5] * len(r[at:at + n])
        reads.append(np.array(r, np.uint8))
    return reads + H.repetitive_reads(100, seed=71, max_len=40)


def callers_stream():
    """locate_dev on a torch stream: input, launch, the caller's own kernel behind it and the read-back are queued on that stream, and
    the host waits once, at the end"""
    import torch
    torch.cuda.init()
    st = torch.cuda.Stream()
    FILL = -7
    g = HipBwt(1)
    for seed in (41, 42):
        g.insert_multi(H.encode_batch(H.repetitive_reads(300, seed=seed, max_len=40), True, True))
    fm = Q.FM(g.bwt())
    g.build_ssa(4)
    rng = np.random.RandomState(9)
    lo = rng.randint(0, fm.N - 8, size=300)
    iv = np.stack([lo, lo + rng.randint(0, 8, size=300)], 1).astype(np.int64)
    w_stored, w_hit, w_cnt = LR.locate_raw(fm, iv, 4)
    g.L.rb2_hip_use_stream(g.h, st.cuda_stream)
    with torch.cuda.stream(st):
        h_iv = torch.from_numpy(iv).pin_memory()
        h_hit = torch.empty((300, 4, 2), dtype=torch.int64).pin_memory()
        h_cnt = torch.empty((300,), dtype=torch.int64).pin_memory()
        h_sum = torch.empty((1,), dtype=torch.int64).pin_memory()
        d_iv = h_iv.to("cuda", non_blocking=True)
        d_hit = torch.full((300, 4, 2), FILL, dtype=torch.int64, device="cuda")
        d_cnt = torch.full((300,), FILL, dtype=torch.int64, device="cuda")
        g.locate_dev(300, d_iv.data_ptr(), d_hit.data_ptr(), d_cnt.data_ptr(), 4)
        d_sum = torch.clamp(d_cnt, max=4).sum().reshape(1)          # the caller's own work behind the engine's, on the same stream
        h_hit.copy_(d_hit, non_blocking=True)
        h_cnt.copy_(d_cnt, non_blocking=True)
        h_sum.copy_(d_sum, non_blocking=True)
    st.synchronize()                                                # the only wait
    live = np.arange(4)[None, :] < w_cnt[:, None]
    assert int(h_sum[0]) == w_stored and np.array_equal(h_cnt.numpy(), w_cnt)
    assert np.array_equal(h_hit.numpy()[live], w_hit[live]) and (h_hit.numpy()[~live] == FILL).all()
    g.close()
    print("STAGE OK")


def main():
    stage = sys.argv[1]
    if stage == "stream":
        return callers_stream()
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)

    def handler(user, msg):
        sys.stdout.write("handler: " + msg.decode())
        sys.stdout.flush()
        os._exit(7)

    cb = CB(handler)
    b1 = H.encode_batch(H.repetitive_reads(300, seed=31, max_len=40), True, True)
    b2 = H.encode_batch(H.repetitive_reads(200, seed=32, max_len=40), True, False)
    if stage == "before":                                           # locate on an index that never had an array
        g = HipBwt(0)
        g.L.rb2_hip_set_fatal_handler(cb, None)
        g.insert_multi(b1)
        print("info", g.ssa_info(), flush=True)
        g.locate_raw([(0, 1)], 1)
        print("NOT FATAL")
    elif stage == "stale":                                          # an insert drops the array: locate is fatal again
        g = HipBwt(0)
        g.L.rb2_hip_set_fatal_handler(cb, None)
        g.insert_multi(b1)
        g.build_ssa(3)
        print("built", g.ssa_info(), flush=True)
        print("located", g.locate_raw([(0, 4)], 4)[2].tolist(), flush=True)
        g.insert_multi(b2)
        print("after insert", g.ssa_info(), flush=True)
        g.locate_raw([(0, 1)], 1)
        print("NOT FATAL")
    elif stage == "life":
        g = HipBwt(0)
        g.L.rb2_hip_set_fatal_handler(cb, None)
        assert g.build_ssa(5) == 0                                  # an empty index: no samples, a valid array
        inf = g.ssa_info()
        assert inf["valid"] and inf["samples"] == 0 and inf["log2_step"] == 5, inf
        stored, hit, cnt = g.locate_raw([(0, 0), (0, 1)], 2)
        assert stored == 0 and cnt.tolist() == [0, -1] and (hit == 0).all()
        g.insert_multi(b1)
        assert not g.ssa_info()["valid"]
        fm1 = Q.FM(g.bwt())
        assert g.build_ssa(3) == (fm1.N + 7) // 8
        all_rows(g, fm1)
        g.insert_multi(b2)                                          # the index grows: the array is gone, a new one answers for the larger index
        inf = g.ssa_info()
        assert not inf["valid"] and inf["device_bytes"] == 0 and inf["samples"] == 0, inf
        fm2 = Q.FM(g.bwt())
        assert fm2.N > fm1.N
        assert g.build_ssa(3) == (fm2.N + 7) // 8
        all_rows(g, fm2)
        n_str = int(fm2.C[1])
        inf = g.ssa_info()
        assert inf["valid"] and inf["log2_step"] == 3 and inf["device_bytes"] == 16 * inf["samples"] + 16 * n_str, inf
        assert g.build_ssa(0) == fm2.N and g.ssa_info()["device_bytes"] == 16 * fm2.N + 16 * n_str   # building again replaces it
        all_rows(g, fm2)
        g.drop_ssa()                                                # frees it
        inf = g.ssa_info()
        assert not inf["valid"] and inf["device_bytes"] == 0, inf
        for what in ("reset", "load_ropes", "load_fmd"):            # the other ways the rows change
            g.build_ssa(4)
            assert g.ssa_info()["valid"]
            if what == "reset":
                g.reset()
            elif what == "load_ropes":
                from ropebwt2_amd.hipbwt import encode_runs
                C1 = np.concatenate([fm1.C, [fm1.N]])
                g.load_ropes([encode_runs(fm1.bwt[C1[b]:C1[b + 1]]) for b in range(6)])
            else:
                import fmd_ref
                g.load_fmd(np.frombuffer(fmd_ref.fixture("rand300")[0], np.uint8))
            inf = g.ssa_info()
            assert not inf["valid"] and inf["device_bytes"] == 0, (what, inf)
        g.close()
        # a re-layout alone keeps the array: the rows stay, the leaves move.  An index grown in place (sparse), an array built on it, then
        # a checksum, which leaves the sparse layout without an insert (ensure_dense): still valid, the same answers
        os.environ.update(FORCED)
        g = HipBwt(1)
        g.L.rb2_hip_set_fatal_handler(cb, None)
        o = H.Oracle(1)
        reads = sparse_reads()
        for part in (reads[:50], reads[50:100], reads[100:]):
            buf = H.encode_batch(part, True, True)
            o.insert_multi(buf); g.insert_multi(buf)
        fm = Q.FM(o.bwt())
        o.close()
        st0 = g.layout_stats()
        assert st0["sparse_now"], st0
        g.build_ssa(5)
        a = all_rows(g, fm)
        assert g.layout_stats() == st0, "locate changed the layout"
        g.rope_hashes()
        st1 = g.layout_stats()
        assert not st1["sparse_now"] and st1["relayouts"] == st0["relayouts"] + 1, (st0, st1)
        assert g.ssa_info()["valid"]
        assert np.array_equal(all_rows(g, fm), a)
        g.close()
        print("STAGE OK")
    else:
        raise SystemExit("unknown stage " + stage)


if __name__ == "__main__":
    main()
