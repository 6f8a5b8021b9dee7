"""CPU tests of the boundary of rb2_hip_approx_ed[_dev]: librb2hip.so exports them with the arguments include/rb2_hip.h gives them, HipBwt
has the methods, MultiBwt has none, the header states the contract, and the kernel is in the gfx950 code object in both layouts.  The
arithmetic is in tests/test_edit_plan.py, the model in tests/test_approx_ed_ref.py, the results in tests/test_approx_ed_gpu.py.  No GPU
needed."""
import ctypes as C
import os
import re

import helpers as H


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS, MultiBwt
    build_all()
    L = load_hip_lib()
    for s, nargs, res in (("rb2_hip_approx_ed", 10, C.c_int64), ("rb2_hip_approx_ed_dev", 10, None)):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        assert len(getattr(L, s).argtypes) == nargs and getattr(L, s).restype is res, s
        assert getattr(L, s).argtypes[4] is C.c_int32                # max_ed is an int, as max_mm is
    for m in ("approx_ed_raw", "approx_ed", "approx_ed_dev"):
        assert callable(getattr(HipBwt, m, None)), m
        assert not hasattr(MultiBwt, m), m                          # a sharded index has none: no method that would only raise


def test_header_states_the_contract():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("---- approximate search with insertions and deletions"):txt.index("void    rb2_hip_approx_ed_dev(")]
    assert txt.index("void    rb2_hip_approx_dev(") < txt.index("---- approximate search with insertions and deletions")       # after the rb2_hip_approx section
    for word in ("ed(S, q)", "sub(", "lev(", "len", "cnt <= -2", "max_ed", "8192", "RB2_APPROX_SCRATCH", "RB2_QUERY_CHUNK", "sharded index", "exactly once",
                 "L - max_ed <= len <= L + max_ed", "max_ed outside 0 .. 4", "n <= 0 returns first", "(lo, hi, 0, L)", "ed <= n_mm"):
        assert word in sec, word
    assert re.search(r"int64_t rb2_hip_approx_ed\(rb2_hip_t \*h, int64_t n, const uint8_t \*qry, const int64_t \*off, int max_ed, int64_t min_occ, int64_t max_steps, "
                     r"int64_t max_recs, int64_t \*rec, int64_t \*cnt\);", txt)
    assert re.search(r"void +rb2_hip_approx_ed_dev\(rb2_hip_t \*h, int64_t n, const uint8_t \*qry, const int64_t \*off, int max_ed, int64_t min_occ, int64_t max_steps, "
                     r"int64_t max_recs, int64_t \*rec, int64_t \*cnt\);", txt)


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    data = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_approx_edILb0E", b"k_approx_edILb1E", b"k_approxILb0E", b"k_approxILb1E"):
        assert k in data, k
