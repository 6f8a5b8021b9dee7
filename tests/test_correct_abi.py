"""CPU tests of the boundary of rb2_hip_correct[_dev] and rb2_hip_correct_into: librb2hip.so exports them with the arguments
include/rb2_hip.h gives them, HipBwt has the methods, MultiBwt has none, the header states the rule, and the kernels are in the gfx950
code object in both layouts.  The rule is in tests/test_correct_plan.py, the model in tests/test_correct_ref.py, the results in
tests/test_correct_gpu.py.  No GPU needed."""
import ctypes as C
import os
import re

import helpers as H


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS, MultiBwt
    build_all()
    L = load_hip_lib()
    for s, nargs, res in (("rb2_hip_correct", 11, C.c_int64), ("rb2_hip_correct_dev", 12, None), ("rb2_hip_correct_into", 9, C.c_int64)):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        assert len(getattr(L, s).argtypes) == nargs and getattr(L, s).restype is res, s
    for m in ("correct_raw", "correct", "correct_dev", "correct_into", "corrected"):
        assert callable(getattr(HipBwt, m, None)), m
        assert not hasattr(MultiBwt, m), m                          # a sharded index has none: no method that would only raise
    assert HipBwt.correct_default_probes() == 101 + 32 * 24 and len(HipBwt.CORRECT_INFO) == 8


def test_header_states_the_definitions():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("---- correcting reads by the k-mer spectrum"):txt.index("int64_t rb2_hip_correct_into(rb2_hip_t *dst")]
    for word in ("WINDOW", "CLEAN", "SOLID", "WEAK", "PROBE", "OVER BUDGET", "PROFILE", "exactly ONE", "L < k", "cnt == -1", "cnt <= -2", "8192", "RB2_QUERY_CHUNK",
                 "RB2_CORRECT_ROWS", "RB2_MERGE_BATCH", "out == qry", "dst == src", "different devices", "sharded index", "batch_bytes < 0", "UNCHANGED", "odd number"):
        assert word in sec, word
    assert re.search(r"int64_t rb2_hip_correct\(rb2_hip_t \*h, int64_t n, const uint8_t \*qry, const int64_t \*off, int64_t k, int64_t min_occ, int64_t max_fix, "
                     r"int64_t max_probes, uint8_t \*out, int64_t \*cnt, int64_t \*weak\);", txt)
    assert re.search(r"void +rb2_hip_correct_dev\(rb2_hip_t \*h, int64_t n, const uint8_t \*qry, const int64_t \*off, int64_t total, int64_t k, int64_t min_occ, "
                     r"int64_t max_fix, int64_t max_probes,\s+uint8_t \*out, int64_t \*cnt, int64_t \*weak\);", txt)
    assert re.search(r"int64_t rb2_hip_correct_into\(rb2_hip_t \*dst, rb2_hip_t \*src, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, int pairs, "
                     r"int64_t batch_bytes, int64_t info\[8\]\);", txt)


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    data = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_correctILb0ELb0", b"k_correctILb1ELb0", b"k_correctILb0ELb1", b"k_correctILb1ELb1", b"k_correct_mate", b"k_correct_reverse"):
        assert k in data, k
