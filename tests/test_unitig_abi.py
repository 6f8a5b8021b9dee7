"""CPU tests of the boundary of the unitig calls: librb2hip.so exports the four entry points with the arguments include/rb2_hip.h gives
them, HipBwt has the methods, MultiBwt has none, and the kernels are in the gfx950 code object.  The launch arithmetic of these calls is a
handful of lines in csrc/rb2_query_host.h (no plan header, so no stand-alone program); the fatal argument checks need a handle, and a
handle needs a device: they are in tests/test_unitig_gpu.py.  No GPU needed."""
import os

import helpers as H


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS, MultiBwt
    build_all()
    L = load_hip_lib()
    for s, nargs in (("rb2_hip_unitig_chains", 6), ("rb2_hip_unitig_chains_dev", 6), ("rb2_hip_unitig_text", 10), ("rb2_hip_unitig_text_dev", 10)):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        assert len(getattr(L, s).argtypes) == nargs, s
    for m in ("unitig_chains", "unitig_chains_dev", "unitig_text", "unitig_text_dev", "unitigs"):
        assert callable(getattr(HipBwt, m, None)), m
        assert not hasattr(MultiBwt, m), m


def test_header_states_the_definitions():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("---- unitigs"):txt.index("rb2_hip_unitig_text_dev(")]
    for word in ("IGNORED", "LINK", "CHAINS", "HEAD", "CLOSING LINK", "SHORT PIECE", "SELECTED", "STORED", "synchronises"):
        assert word in sec, word


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    data = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_unitig_deg", b"k_unitig_link", b"k_unitig_jump", b"k_unitig_sum", b"k_unitig_text"):
        assert k in data, k
