"""Float BAM tags in the FASTQ header lines, the rule (bam.float_g; tag_comment / fastq_text_tagged / tag_counts with floats=True; the
CLI's --bam_tag_floats): float_g against this C library's printf("%g") and against literals written by hand. No GPU."""
import ctypes
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_float_cases as F  # noqa: E402
import bam_tagtext_cases as TC  # noqa: E402
import bam_tags_cases as T  # noqa: E402
from fractions import Fraction  # noqa: E402
from ribodetector_amd import bam  # noqa: E402


def _glibc(patterns):
    """snprintf("%g", (double)v) of every pattern"""
    libc = ctypes.CDLL(None)
    libc.snprintf.restype = ctypes.c_int
    libc.snprintf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_double]
    buf = ctypes.create_string_buffer(64)
    floats = struct.unpack("<%df" % len(patterns), struct.pack("<%dI" % len(patterns), *patterns))     # (float -> double is exact)
    out = []
    for b, f in zip(patterns, floats):
        if (b & 0x7fffffff) > F.INF:                      # a NaN: struct may have touched the payload, the text does not depend on it
            f = float("nan") if not b >> 31 else -float("nan")
        n = libc.snprintf(buf, 64, b"%g", f)
        out.append(buf.raw[:n])
    return out


def _same(got, want, patterns):
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("0x%08x: %r != %r" % (patterns[k], got[k], want[k]))


@pytest.mark.parametrize("which", ["hard", "sweep", "random"])
def test_float_g_is_printf_g(which):
    patterns = {"hard": F.hard, "sweep": lambda: F.sweep(1, 64), "random": lambda: F.randoms(3, 1 << 18)}[which]()
    got = F.rule_texts(which, patterns)
    want = _glibc(patterns)
    _same(got, want, patterns)
    assert max(len(t) for t in got) <= 12
    if which == "hard":
        assert max(len(t) for t in got) == 12 and bam.float_g(F.FLT_MIN | F.SIGN) == b"-1.17549e-38"


def test_float_g_is_pythons_g_but_for_the_sign_of_nan():
    patterns = F.sweep(4, 16) + F.randoms(5, 1 << 16) + F.NANS + F.hard()[:8000]
    floats = struct.unpack("<%df" % len(patterns), struct.pack("<%dI" % len(patterns), *patterns))
    for b, f in zip(patterns, floats):
        want = ("%g" % f).encode()
        if (b & 0x7fffffff) > F.INF:
            assert want == b"nan" and bam.float_g(b) == (b"-nan" if b >> 31 else b"nan")
        else:
            assert bam.float_g(b) == want, hex(b)


def test_ties_go_to_the_even_digit():
    for v, want in F.TIE_LITERALS:
        b = F.exact(Fraction(v))
        assert b is not None, v                           # (an exact tie: the float IS the number written here)
        assert bam.float_g(b) == want, v
    for v, want in F.LITERALS:
        assert bam.float_g(F.bits_of(Fraction(v))) == want, v
    # and every tie of the search: the 6th digit of the text is even
    t = F.ties()
    seven = t["n5"][:900000]                              # (in rising order: the whole numbers of 7 digits)
    assert F.value_of(seven[0]) == 1000005 and F.value_of(seven[-1]) == 9999995 and len(t["big"]) > 100000 and len(t["half"]) > 3000
    for b in seven[::7] + t["big"][::5] + t["half"]:
        text = bam.float_g(b)
        mant = text.split(b"e")[0].replace(b".", b"")
        assert b"e" in text or len(mant) == 6, text        # (without an exponent: a k + 0.5, which prints as a whole number of 6 digits)
        assert (mant.ljust(6, b"0")[5] - 48) % 2 == 0, (hex(b), text)


def _one(tags, lst, floats):
    data = TC.file_data([T.rec(tags, name=b"r")])
    return bam.tag_comment(data, len(bam.encode_header()), lst, floats=floats)


def test_tag_comment_with_floats():
    for name, tags, lst, on, off in F.tagged_cases():
        comment, copied, mal, fl = _one(tags, lst, True)
        assert comment == on and not mal and fl == 0, name
        assert copied == [(b"\t" + t + b":") in on for t in lst], name
        comment, copied, mal, fl = _one(tags, lst, False)
        assert comment == off and not mal, name
        assert (comment, copied, mal, fl) == bam.tag_comment(TC.file_data([T.rec(tags, name=b"r")]), len(bam.encode_header()), lst), name
    for name, tags, lst in F.MALFORMED_CASES:
        for floats in (False, True):
            assert _one(tags, lst, floats) == (b"", [False] * len(lst), True, 0), name
    # a float value counts as skipped only without the flag
    assert _one(F.f_tag(b"qs", F.bits_of(12.5)), [b"qs"], False)[3] == 1 and _one(F.bf_tag(b"XF", [1, 2]), [b"XF"], False)[3] == 1


def test_floats_off_is_what_it_was():
    """every existing case and the random records: floats=False is the call without the keyword; floats=True changes nothing but the
    float tags"""
    for k, (name, tags, lst, want) in enumerate(TC.CASES):
        data = TC.file_data([TC.case_record(k, tags)])
        off = len(bam.encode_header())
        assert bam.tag_comment(data, off, lst, floats=False) == bam.tag_comment(data, off, lst), name
        assert bam.tag_comment(data, off, lst)[0] == (b"" if want == TC.MALFORMED else want), name
        if name not in TC.FLOATS:
            assert bam.tag_comment(data, off, lst, floats=True) == bam.tag_comment(data, off, lst), name
    recs, lst = TC.random_records(2, 400)
    data = TC.file_data(recs)
    assert bam.fastq_text_tagged(data, lst, floats=False) == bam.fastq_text_tagged(data, lst)
    assert bam.tag_counts(data, lst, floats=False) == bam.tag_counts(data, lst)
    on, off = bam.tag_counts(data, lst, floats=True), bam.tag_counts(data, lst)
    assert off["float_values_skipped"] > 50 and on["float_values_skipped"] == 0 and on["malformed_records"] == off["malformed_records"]
    assert sum(on["copied"]) == sum(off["copied"]) + off["float_values_skipped"]
    text = bam.fastq_text_tagged(data, lst, floats=True)
    assert text.count(b":f:") + text.count(b":B:f") == off["float_values_skipped"]
    assert len(text) > len(bam.fastq_text_tagged(data, lst))


def test_the_flag_needs_the_list():
    from ribodetector_amd import detect
    with pytest.raises(RuntimeError, match=r"--bam_tag_floats.*--bam_tags"):
        detect.check_bam_tags(None, ["x.bam"], floats=True)
    assert detect.check_bam_tags(None, ["x.bam"]) is None and detect.check_bam_tags(None, ["x.bam"], False, floats=False) is None
    assert detect.check_bam_tags("qs,RG", ["x.bam"], floats=True) == [b"qs", b"RG"]
    args = detect.build_parser().parse_args(["-l", "100", "-i", "x.bam", "-o", "o.fq", "--bam_tag_floats"])
    assert args.bam_tag_floats and args.bam_tags is None
    assert not detect.build_parser().parse_args(["-l", "100", "-i", "x.bam", "-o", "o.fq"]).bam_tag_floats
    with pytest.raises(RuntimeError, match=r"--bam_tag_floats.*--bam_tags"):
        detect.main(["-i", "x.bam", "-o", "o.fq", "-l", "100", "--bam_tag_floats"])


def test_to_json_names_the_format_only_when_asked():
    from ribodetector_amd import bamtags
    c = {"copied": [3, 1], "malformed_records": 2, "float_values_skipped": 0}
    base = bamtags.to_json([b"qs", b"RG"], [c])
    assert "float_format" not in base and base == bamtags.to_json([b"qs", b"RG"], [c], floats=False)
    on = bamtags.to_json([b"qs", b"RG"], [c], floats=True)
    assert list(on) == list(base) + ["float_format"] and on["float_format"] == "%g" and {k: on[k] for k in base} == base
    two = bamtags.to_json([b"qs"], [c, c], floats=True)
    assert list(two)[-1] == "float_format" and two["copied"] == [[3, 3]]
    assert bamtags.log_line([b"qs", b"RG"], [c]).endswith("0 float values skipped")
