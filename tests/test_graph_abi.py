"""CPU tests of the boundary of the string-graph call: librb2hip.so exports rb2_hip_string_graph and rb2_hip_string_graph_dev with the
signatures include/rb2_hip.h declares, the header documents them, HipBwt has the methods, and the kernels are in the code object.  The
fatal argument checks need a handle, and a handle needs a device: they are in tests/test_graph_gpu.py.  No GPU needed."""
import ctypes as C
import os
import re

import helpers as H

NAMES = ("rb2_hip_string_graph", "rb2_hip_string_graph_dev")


def _header():
    return open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS
    build_all()
    L = load_hip_lib()
    i64, vp = C.c_int64, C.c_void_p
    for s in NAMES:
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        f = getattr(L, s)
        assert f.restype is i64 and list(f.argtypes) == [vp] + [i64] * 7 + [C.c_int, i64, vp, vp], s
    for m in ("string_graph", "string_graph_dev", "string_graph_raw", "assemble"):
        assert callable(getattr(HipBwt, m, None)), m


def test_header_declares_what_the_library_is_called_with():
    """the declarations, argument by argument: the ctypes signatures above are these"""
    txt = _header()
    for s in NAMES:
        m = re.search(r"int64_t\s+%s\(([^;]*)\);" % s, txt)
        assert m, s
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert args == ["rb2_hip_t *h", "int64_t first", "int64_t n", "int64_t min_ovlp", "int64_t max_ext", "int64_t max_steps", "int64_t max_recs", "int64_t max_hits",
                        "int pairs", "int64_t cap", "int64_t *edges", "int64_t info[8]"], (s, args)


def test_header_documents_the_call():
    txt = _header()
    sec = txt[txt.index("the string graph of the index's own strings"):txt.index("rb2_hip_string_graph_dev(")]
    for word in ("rb2_hip_irreducible", "rb2_hip_string_ids", "REVERSE COMPLEMENT", "id ^ 1", "increasing src", "cap == 0", "RB2_GRAPH_CHUNK", "256 MiB", "RB2_IRRED_SCRATCH",
                 "rb2_hip_ssa_build", "sharded", "max_hits < 1", "odd number of strings", "dense and on the sparse", "synchronises once per chunk"):
        assert word in sec, word
    integ = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
    assert "rb2_hip_string_graph" in integ and "RB2_GRAPH_CHUNK" in integ
    assert "## 23." in open(os.path.join(H.ROOT, "DESIGN.md")).read()


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    blob = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_graph_count", b"k_graph_emit", b"k_graph_cut"):
        assert k in blob, k
