"""CPU tests of the boundary of rb2_hip_unpack[_dev] and rb2_hip_merge: librb2hip.so exports them with the arguments include/rb2_hip.h
gives them, HipBwt has the methods, MultiBwt has none, the header states the definitions, and the unpack kernels are in the gfx950 code
object.  The cutting arithmetic is in tests/test_merge_plan.py, the model in tests/test_merge_ref.py, the results in tests/test_merge_gpu.py.
No GPU needed."""
import ctypes as C
import os
import re

import helpers as H


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS, MultiBwt
    build_all()
    L = load_hip_lib()
    for s, nargs in (("rb2_hip_unpack", 7), ("rb2_hip_unpack_dev", 7), ("rb2_hip_merge", 4)):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        assert len(getattr(L, s).argtypes) == nargs and getattr(L, s).restype is C.c_int64, s
    for m in ("unpack_raw", "unpack", "unpack_dev", "merge"):
        assert callable(getattr(HipBwt, m, None)), m
        assert not hasattr(MultiBwt, m), m                          # a sharded index has neither: no method that would only raise


def test_header_states_the_definitions():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("---- the strings of the index, packed"):txt.index("rb2_hip_merge(rb2_hip_t *dst")]
    for word in ("SIZE", "reversed != 0", "reversed == 0", "writes NOTHING", "UNCHANGED", "Fatal", "RB2_MERGE_BATCH", "RB2_QUERY_CHUNK", "256 MiB",
                 "dst == src", "different devices", "sharded index", "cap < 0", "batch_bytes < 0", "first + n", "no BWT", "synchronises"):
        assert word in sec, word
    assert re.search(r"int64_t rb2_hip_unpack\(rb2_hip_t \*h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t \*txt, int64_t \*off\);", txt)
    assert re.search(r"int64_t rb2_hip_unpack_dev\(rb2_hip_t \*h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t \*txt, int64_t \*off\);", txt)
    assert re.search(r"int64_t rb2_hip_merge\(rb2_hip_t \*dst, rb2_hip_t \*src, int64_t batch_bytes, int64_t info\[4\]\);", txt)


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    data = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_unpack_lenILb0", b"k_unpack_lenILb1", b"k_unpack_textILb0", b"k_unpack_textILb1"):
        assert k in data, k
