"""The owner and the layout of call scratch (csrc/rb2_scratch.h) without a GPU.  CallScope: a normal return, an exception through two nested
scopes, release_open() followed by a longjmp past both frames and by the destructors, a scope of a second thread, a buffer that grew.  Carve: the
four layouts of the query host layer at n in {0, 1, 2, 3, 4097} and m in {0, 1, 5, 4096} -- the counting pass against the closed formulas, every
region inside the buffer, 8-aligned and disjoint (each filled with a tag of its own and read back), a layout whose passes differ, sizes that
would wrap.  CPU only: tests/scratch_check.cpp includes the header over malloc'ed buffers and is run as a program of its own, once plain and
once under AddressSanitizer (with its leak check) + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "ropebwt2_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O3"], SAN], ids=["plain", "sanitized"])
def test_call_scope_and_carve(tmp_path, flags):
    exe = str(tmp_path / "scratch_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "scratch_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode()[-3000:]
    assert p.returncode == 0 and out.startswith("SCRATCH OK"), (p.returncode, out, err)
    assert "ERROR: AddressSanitizer" not in err and "ERROR: LeakSanitizer" not in err and "runtime error" not in err, err
    layouts, regions = (int(out.split()[i]) for i in (5, 7))
    # chains, text and graph at five n; clean at five n x four m.  Regions: chains 7, text 12, graph 5, clean 7 + 16
    assert layouts == 5 * 3 + 5 * 4
    assert regions == 5 * (7 + 12 + 5) + 20 * 23
