"""The formatter the kernels run (csrc/rd_float_text.hpp: ft_format, plain C++ over integers) compiled for the host and compared with
the rule bam.float_g - the same arithmetic as on the device, checked without one. tests/float_text_host.cpp is the program."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_float_cases as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("float_text") / "float_text_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "float_text_host.cpp")], check=True)
    return exe


def test_host_build_of_the_formatter_is_the_rule(program, tmp_path):
    patterns = F.hard() + F.sweep(2, 64) + F.randoms(7, 1 << 18)
    want = F.rule_texts("hard", F.hard()) + F.rule_texts("sweep2+random7", patterns[len(F.hard()):])
    src, dst = str(tmp_path / "bits"), str(tmp_path / "text")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<%dI" % len(patterns), *patterns))
    subprocess.run([program, src, dst], check=True)
    got = open(dst, "rb").read()
    assert len(got) == 17 * len(patterns)
    for k, w in enumerate(want):
        slot = got[17 * k:17 * k + 17]
        if slot != w.ljust(16, b"\0") + bytes([len(w)]):
            raise AssertionError("0x%08x: %r, want %r" % (patterns[k], slot, w))


def test_host_build_against_the_c_library_on_a_stride_of_all_patterns(program):
    """every 4099th of the 2^32 patterns (a prime stride: every exponent field, about 4,000 mantissas each) against snprintf("%g")"""
    r = subprocess.run([program, "--self", "0", str(1 << 32), "4099"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches, longest 12" in r.stdout, r.stdout[-2000:]
