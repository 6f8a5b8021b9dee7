"""CPU test of the boundary of string deletion: the library exports rb2_hip_delete_strings and rb2_hip_delete_stats with the signatures
the Python mirror binds, the header declares them, and HipBwt has the method.  No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re

import helpers as H


def test_delete_is_exported_and_bound():
    from ropebwt2_amd import HipBwt, MultiBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS
    build_all()
    lib = load_hip_lib()
    f = lib.rb2_hip_delete_strings
    assert f.restype is C.c_int64 and list(f.argtypes) == [C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.rb2_hip_delete_stats.restype is None
    assert "rb2_hip_delete_strings" in ABI_SYMBOLS and "rb2_hip_delete_stats" in ABI_SYMBOLS
    assert callable(HipBwt.delete) and callable(HipBwt.delete_stats)
    assert not hasattr(MultiBwt, "delete")                          # a sharded index has no deletion: no method that would only raise
    hdr = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    assert re.search(r"int64_t\s+rb2_hip_delete_strings\(rb2_hip_t \*h, int64_t n, const int64_t \*ids\);", hdr)
