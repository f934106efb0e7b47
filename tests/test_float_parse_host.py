"""The decimal -> float32 rule of --ubam_tag_floats (bam.float_from_text) on its case tables and against a second statement of it in
Fractions; its two guarantees; and the scanner and converter the kernels run (csrc/rd_float_parse.hpp: fp_scan, fp_round, plain C++
over integers) compiled for the host and compared with the rule - the same arithmetic as on the device, checked without one.
tests/float_parse_host.cpp is the program; a second build of it runs under the address and undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_float_cases as F  # noqa: E402
import float_parse_cases as C  # noqa: E402
import ubam_tag_float_cases as U  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_rule_on_the_hard_cases():
    assert bam.FLOAT_SKIPPED == C.SKIPPED and bam.FLOAT_DIGITS == 17
    for text, want in C.HARD:
        assert bam.float_from_text(text) == want, text


def test_the_rule_on_the_syntax_table():
    for text, ok in C.SYNTAX:
        assert (bam.float_from_text(text) is not None) == ok, text
        assert (bam.float_from_text(b"-" + text) is not None) == (ok and text[:1] not in (b"+", b"-")), text


def test_the_rule_is_the_nearest_float_by_exact_comparison():
    """a statement of the rule that shares no code with it: bisection over the bit patterns with Fractions"""
    for M, q, neg, text in C.random_texts(11, 4000):
        assert bam.float_from_text(text) == C.by_fractions(M, q, neg), text
    for text, want in C.HARD:
        if want is not None and want != C.SKIPPED and want & 0x7fffffff < C.INF and want & 0x7fffffff:
            m = bam._FLOAT_TEXT.fullmatch(text)
            digits = (m.group(2) or m.group(3) + m.group(4)).lstrip(b"0") or b"0"
            q = int(m.group(5) or 0) - len(m.group(4) or b"")
            assert C.by_fractions(int(digits), q, text[:1] == b"-") == want, text


def test_the_rule_at_the_midpoints():
    for text, want in C.midpoint_texts(4, 6) + C.exact_midpoints():
        assert bam.float_from_text(text) == want, text


def _patterns():
    return F.hard() + F.sweep(2, 20) + F.randoms(7, 1 << 16)


def test_guarantee_b_nine_and_seventeen_digits_give_the_bits_back():
    for fmt in ("%.9g", "%.17g"):
        texts, patterns = C.pattern_texts(_patterns(), fmt)
        assert C.rule(fmt, texts) == patterns


def test_guarantee_a_the_g_text_is_a_fixed_point():
    """float_g . float_from_text . float_g == float_g on every pattern, NaNs and infinities included (a NaN keeps its sign only)"""
    patterns = _patterns()
    texts = F.rule_texts("parse:hard+sweep2x20+random7", patterns)
    back = C.rule("g of patterns", texts)
    for b, t, r in zip(patterns, texts, back):
        assert r is not None and r != C.SKIPPED and bam.float_g(r) == t, hex(b)
        if (b >> 23) & 0xff == 0xff and b & 0x7fffff:
            assert r == (b & C.SIGN) | C.NAN


def test_the_size_bound_over_the_case_table():
    """a field of t text bytes makes at most max(t, 2 t - 4) tag bytes: XY:f:v is t >= 6 for 7, XY:B:f with n elements t >= 6 + 2 n for
    8 + 4 n - so bam.ubam_bound holds the records of any text whose comments hold float fields only"""
    seen = 0
    for name, comment, tags, want, _ in U.CASES:
        for field in comment.split(b"\t"):
            got = bam.tags_from_comment(b"@r " + field, tags, floats=True)[0]
            assert len(got) <= max(len(field), 2 * len(field) - 4), name
            seen += bool(got)
    assert seen > 20
    for n in (0, 1, 2, 300):
        field = b"XF:B:f" + b",1" * n
        assert len(bam.tags_from_comment(b"@r " + field, [b"XF"], floats=True)[0]) == 8 + 4 * n <= max(len(field), 2 * len(field) - 4)
    text = U.fastq([(b"r%d" % k, c) for k, (_, c, _, _, _) in enumerate(U.CASES)])
    tags = sorted({t for _, _, ts, _, _ in U.CASES for t in ts})[:bam.TAGS_MAX]
    assert len(bam.from_fastq(text, tags=tags, floats=True)) <= bam.ubam_bound(len(text), len(U.CASES))


def _build(tmp_path_factory, name, extra):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / "float_parse_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, os.path.join(HERE, "float_parse_host.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "float_parse", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "float_parse_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, texts, tmp_path, tag):
    src, dst = str(tmp_path / ("texts" + tag)), str(tmp_path / ("bits" + tag))
    with open(src, "wb") as fh:
        fh.write(b"".join(struct.pack("<I", len(t)) + t for t in texts))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = open(dst, "rb").read()
    assert len(got) == 5 * len(texts)
    return [struct.unpack_from("<IB", got, 5 * k) for k in range(len(texts))]


def _want(r):
    return (0, 1) if r is None else (0, 2) if r == C.SKIPPED else (r, 0)


def _table_texts():
    texts = [t for t, _ in C.HARD] + [t for t, _ in C.SYNTAX] + [b"-" + t for t, _ in C.SYNTAX]
    texts += [t for t, _ in C.midpoint_texts(4, 6) + C.exact_midpoints()]
    return texts


def test_host_build_is_the_rule(program, tmp_path):
    """(i): the tables, the three printed forms of the patterns, the midpoints and 2^18 generated texts"""
    texts = _table_texts()
    want = C.rule("tables", texts)
    for fmt in ("%g", "%.9g", "%.17g"):
        t, _ = C.pattern_texts(_patterns(), fmt)
        texts, want = texts + t, want + C.rule("patterns " + fmt, t)
    gen = [t for _, _, _, t in C.random_texts(13, 1 << 18)]
    texts, want = texts + gen, want + C.rule("random13", gen)
    got = _run(program, texts, tmp_path, "")
    for t, g, w in zip(texts, got, want):
        assert g == _want(w), t


def test_host_build_under_the_sanitizers(sanitized, tmp_path):
    """the same program built with -fsanitize=address,undefined: every buffer holds its text and not a byte more, so a read at or
    behind a value's end, a shift by a bad count or a signed overflow ends the run"""
    texts = _table_texts() + [t for _, _, _, t in C.random_texts(17, 1 << 14)]
    want = C.rule("tables", _table_texts()) + C.rule("random17", texts[len(_table_texts()):])
    got = _run(sanitized, texts, tmp_path, "_san")
    for t, g, w in zip(texts, got, want):
        assert g == _want(w), t
    r = subprocess.run([sanitized, "--self", "0", str(1 << 32), "1000003"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_host_build_against_the_c_library_on_a_stride_of_all_patterns(program):
    """(ii): every 4099th of the 2^32 patterns (a prime stride: every exponent field, about 4,000 mantissas each), printed with %.9g
    and with %g, against strtof of the same text - and the %.9g text gives the pattern itself back. That this C library's strtof is
    correctly rounded is recalled, not verified here: where the two disagree the rule stands."""
    r = subprocess.run([program, "--self", "0", str(1 << 32), "4099"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-2000:]
