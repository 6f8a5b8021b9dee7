"""CPU tests of the boundary of the graph-cleaning call: librb2hip.so exports rb2_hip_graph_clean and rb2_hip_graph_clean_dev with the
signatures include/rb2_hip.h declares, the header documents them, HipBwt has the methods, and the kernels are in the code object.  The
fatal argument checks need a handle, and a handle needs a device: they are in tests/test_graph_clean_gpu.py.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import helpers as H

NAMES = ("rb2_hip_graph_clean", "rb2_hip_graph_clean_dev")


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
        assert f.restype is i64 and list(f.argtypes) == [vp, i64, i64, vp, i64, i64, C.c_int, i64, i64, vp, vp], s
    for m in ("graph_clean", "graph_clean_dev", "graph_clean_raw", "assemble"):
        assert callable(getattr(HipBwt, m, None)), m
    sig = inspect.signature(HipBwt.graph_clean).parameters
    assert [(k, sig[k].default) for k in ("n_str", "max_tip_reads", "max_bubble_reads", "pairs", "max_rounds")] == \
        [("n_str", None), ("max_tip_reads", 2), ("max_bubble_reads", 3), ("pairs", True), ("max_rounds", 8)]
    assert inspect.signature(HipBwt.assemble).parameters["clean"].default is None


def test_header_declares_what_the_library_is_called_with():
    """the declarations, argument by argument: the ctypes signatures above are these"""
    txt = _header()
    for s in NAMES:
        m = re.search(r"int64_t\s+%s\(([^;]*)\);" % s, txt)
        assert m, s
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert args == ["rb2_hip_t *h", "int64_t n_str", "int64_t m", "const int64_t *edges", "int64_t max_tip_reads", "int64_t max_bubble_reads", "int pairs",
                        "int64_t max_rounds", "int64_t cap", "int64_t *out", "int64_t info[8]"], (s, args)


def test_header_documents_the_call():
    txt = _header()
    sec = txt[txt.index("tip and bubble removal on an edge list"):txt.index("rb2_hip_graph_clean_dev(")]
    for word in ("rb2_hip_unitig_chains", "IGNORED", "OUT-TIP", "IN-TIP", "BUBBLE", "ARM", "LOSES", "minpid", "v >> pairs", "lexicographic", "max_rounds", "cap == 0",
                 "must not overlap", "rounds run", "chains of the list as returned", "synchronises once", "9 bytes per row", "187 bytes per vertex", "sharded",
                 "max_recs * max_hits", "before any kernel"):
        assert word in sec, word
    assert "## 24." in open(os.path.join(H.ROOT, "DESIGN.md")).read()
    assert "rb2_hip_graph_clean" in open(os.path.join(H.ROOT, "README.md")).read()


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    blob = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_clean_deg", b"k_clean_sum", b"k_clean_class", b"k_clean_widen", b"k_clean_fill", b"k_clean_rival", b"k_clean_anchor", b"k_clean_mark", b"k_clean_keep",
              b"k_clean_emit"):
        assert k in blob, k
