"""The oracle of the .fmd encoder tests: the host writer of this project (libropebwt2.so: rb2_fmd_*, include/rb2_fmd.h), which restates
rld0.c and is compared with the reference binary elsewhere (tests/test_host_layer.py, tests/test_cli_gpu.py)."""
import ctypes as C

import numpy as np

_host = None


def host_lib():
    global _host
    if _host is None:
        from ropebwt2_amd.build import lib_path
        L = C.CDLL(lib_path("libropebwt2.so"))
        L.rb2_fmd_init.restype = C.c_void_p
        L.rb2_fmd_push.argtypes = [C.c_void_p, C.c_int64, C.c_int]
        L.rb2_fmd_push_runs.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.rb2_fmd_finish.argtypes = [C.c_void_p]
        L.rb2_fmd_write_path.argtypes = [C.c_void_p, C.c_char_p]
        L.rb2_fmd_destroy.argtypes = [C.c_void_p]
        _host = L
    return _host


def write_fmd(path, rles=(), pushes=()):
    """an .fmd from six 43+3 run streams in rope order (and / or single runs (len, sym)); returns the file image"""
    L = host_lib()
    f = L.rb2_fmd_init()
    for r in rles:
        b = np.ascontiguousarray(r, dtype=np.uint8).tobytes()
        L.rb2_fmd_push_runs(f, b, len(b))
    for l, c in pushes:
        L.rb2_fmd_push(f, l, c)
    L.rb2_fmd_finish(f)
    assert L.rb2_fmd_write_path(f, str(path).encode()) == 0
    L.rb2_fmd_destroy(f)
    return np.fromfile(str(path), dtype=np.uint8)


def fmd_of(g, path):
    """the image the host route gives for the index of handle g"""
    return write_fmd(path, [g.rope_rle(b) for b in range(6)])
