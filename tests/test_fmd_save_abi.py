"""CPU tests of the boundary of the .fmd encoder: librb2hip.so exports the two entry points with the arguments include/rb2_hip.h gives them,
HipBwt has the method, MultiBwt has none, the header states the definitions, and the kernels are in the gfx950 code object.  The arithmetic
is in tests/test_fmd_plan.py, the images in tests/test_fmd_save_gpu.py.  No GPU needed."""
import os

import helpers as H


def test_symbols_and_methods():
    from ropebwt2_amd import HipBwt, build_all, load_hip_lib
    from ropebwt2_amd.hipbwt import ABI_SYMBOLS, MultiBwt
    build_all()
    L = load_hip_lib()
    for s, nargs in (("rb2_hip_save_fmd", 3), ("rb2_hip_save_fmd_file", 2)):
        assert hasattr(L, s) and s in ABI_SYMBOLS, s
        assert len(getattr(L, s).argtypes) == nargs, s
    assert callable(getattr(HipBwt, "save_fmd", None))
    assert not hasattr(MultiBwt, "save_fmd")


def test_header_states_the_definitions():
    txt = open(os.path.join(H.ROOT, "include", "rb2_hip.h")).read()
    sec = txt[txt.index("---- the index as an .fmd image"):txt.index("rb2_hip_save_fmd_file(")]
    for word in ("SIZE", "NOTHING", "UNCHANGED", "EMPTY", "synchronises", "RB2_FMDS_SEG"):
        assert word in sec, word


def test_kernels_are_in_the_code_object():
    from ropebwt2_amd import build_all
    from ropebwt2_amd.build import lib_path
    build_all()
    data = open(lib_path("librb2hip.so"), "rb").read()
    for k in (b"k_fmds_heads", b"k_scan_part", b"k_scan_top", b"k_scan_apply", b"k_fmds_next", b"k_fmds_table", b"k_fmds_group", b"k_fmds_resolve",
              b"k_fmds_down", b"k_fmds_write", b"k_fmds_hdrfix", b"k_fmds_carry", b"k_fmds_frames"):
        assert k in data, k
