"""CPU test of the boundary of the duplicate / containment query: the library exports rb2_hip_contained and rb2_hip_contained_dev with the
signatures the Python mirror binds, the header declares them, HipBwt has the four methods and MultiBwt none of them.  No compute calls
(there is no GPU here)."""
import ctypes as C
import os
import re

import helpers as H


def test_contained_is_exported_and_bound():
    from ropebwt2_amd import HipBwt, MultiBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS
    build_all()
    lib = load_hip_lib()
    f, d = lib.rb2_hip_contained, lib.rb2_hip_contained_dev
    assert f.restype is C.c_int64 and list(f.argtypes) == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert d.restype is None and list(d.argtypes) == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert "rb2_hip_contained" in ABI_SYMBOLS and "rb2_hip_contained_dev" in ABI_SYMBOLS
    for name in ("contained_raw", "contained_dev", "contained", "reduce"):
        assert callable(getattr(HipBwt, name))
        assert not hasattr(MultiBwt, name)                          # a sharded index has no queries: no method that would only raise
    hdr = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    assert re.search(r"int64_t\s+rb2_hip_contained\(rb2_hip_t \*h, int64_t n, const int64_t \*ids, int64_t \*rec\);", hdr)
    assert re.search(r"void\s+rb2_hip_contained_dev\(rb2_hip_t \*h, int64_t n, const int64_t \*ids, int64_t \*rec\);", hdr)
