"""Texts of float values for the decimal -> float32 conversion of --ubam_tag_floats (bam.float_from_text, C ABI rd_float_parse /
rd_bam_encode_ex), shared by tests/test_float_parse_host.py and tests/test_gpu_float_parse.py. A text is bytes; a result is a bit pattern
(an int below 2^32), SKIPPED (more than 17 significant digits) or None (not of the syntax). HARD holds its results by hand; for the
generated texts the yardsticks are the rule and by_fractions, a second statement of it that shares no code with the rule."""
import os
import random
import struct
import sys
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_float_cases as F  # noqa: E402

SKIPPED = -1                     # bam.FLOAT_SKIPPED
INF, SIGN, NAN = 0x7f800000, 0x80000000, 0x7fc00000
OVERFLOW = 2 ** 128 - 2 ** 103   # FLT_MAX plus half an ulp: the least value that is infinity


def g_text(bits, fmt="%g"):
    """the text a C library prints for the float32 with the pattern `bits` (Python's % on the float's exact double is the same)"""
    return (fmt % struct.unpack("<f", struct.pack("<I", bits))[0]).encode()


def _digits17(x):
    """(N, p): the Fraction x > 0 cut to 17 significant digits, N 10^p <= x < (N + 1) 10^p with 10^16 <= N < 10^17"""
    p = len(str(x.numerator // x.denominator)) - 17 if x >= 1 else -17
    while Fraction(10) ** (p + 17) <= x:
        p += 1
    while Fraction(10) ** (p + 16) > x:
        p -= 1
    return int(x / Fraction(10) ** p), p


def _sci(N, p):
    return b"%de%d" % (N, p)


# the issue's table, by hand
HARD = [
    (b"16777217", 0x4b800000), (b"16777219", 0x4b800002), (b"8388608.5", 0x4b000000), (b"8388609.5", 0x4b000002),
    (b"1.0000000596046447", 0x3f800000), (b"1.0000000596046448", 0x3f800001), (b"1.00000005960464478", SKIPPED),
    (b"3.4028235677973366e38", 0x7f7fffff), (b"3.40282e+38", 0x7f7fffee), (b"3.40283e+38", 0x7f800000),
    (b"7.006492321624085e-46", 0x00000000), (b"7.006492321624086e-46", 0x00000001), (b"1e-46", 0x00000000), (b"1e-9999", 0x00000000),
    (b"1e9999", 0x7f800000), (b".5", 0x3f000000), (b"-0", 0x80000000), (b"+inf", 0x7f800000), (b"-NaN", 0xffc00000),
    (b"5.", None), (b"1e", None), (b"1e99999", None),
    # the 17-digit neighbours of 2^128 - 2^103 = 3.40282356779733661637...e38
    (b"3.4028235677973366e38", 0x7f7fffff), (b"3.4028235677973367e38", 0x7f800000), (b"-3.4028235677973367e38", 0xff800000),
    (b"34028235677973366e22", 0x7f7fffff), (b"34028235677973367e22", 0x7f800000),
    # the smallest and largest normal and denormal, %.9g and %g
    (b"1.17549435e-38", 0x00800000), (b"1.17549e-38", 0x007fffe1), (b"3.40282347e+38", 0x7f7fffff), (b"1.40129846e-45", 0x00000001),
    (b"1.4013e-45", 0x00000001), (b"1.17549421e-38", 0x007fffff), (b"-1.17549421e-38", 0x807fffff),
    # leading and trailing zeros are free
    (b"0." + b"0" * 44 + b"1", 0x00000001), (b"0" * 60 + b"1" + b"0" * 60 + b"e-60", 0x3f800000),
    (b"0" * 60 + b"12345678901234567" + b"0" * 60 + b"e-70", 0x4996b43f), (b"0." + b"0" * 60 + b"25" + b"0" * 60 + b"e61", 0x40200000),
    (b"0" * 60 + b"123456789012345678" + b"0" * 60, SKIPPED),
    (b"-0.000e5", 0x80000000), (b"0e9999", 0x00000000), (b"-.0", 0x80000000), (b"1E2", 0x42c80000), (b"+1.5e+0", 0x3fc00000),
    (b"100000000000000000", 0x5bb1a2bc), (b"99999999999999999", 0x5bb1a2bc), (b"999999999999999991", SKIPPED), (b"1e38", 0x7e967699),
    (b"1e39", 0x7f800000), (b"9.9999999999999999e38", 0x7f800000), (b"9.99999999999999999e38", SKIPPED), (b"1e-45", 0x00000001), (b"1e-62", 0x00000000),
    (b"99999999999999999e-62", 0x00000001), (b"99999999999999999e-63", 0x00000000), (b"99999999999999999e22", 0x7f800000),
    (b"99999999999999999e21", 0x7e967699), (b"inf", 0x7f800000), (b"INF", 0x7f800000), (b"-Inf", 0xff800000), (b"nan", 0x7fc00000), (b"+nAn", 0x7fc00000),
]

# (text, is it of the syntax?)
SYNTAX = [(t, False) for t in (
    b"", b" ", b"+", b"-", b".", b"+.", b"e5", b".e5", b"5.", b"5.e3", b"1e", b"1e+", b"1e-", b"1e12345", b"1e+12345", b"0x1p3", b"0x10", b"infinity", b"nan(1)",
    b"in", b"na", b"i", b"infx", b"1 ", b" 1", b"1\t", b"1,2", b"1..2", b"1.2.3", b"--1", b"+-1", b"1e1.5", b"1e5e5", b"1f", b"1.0f", b"1_0", b"\xb1",
    b"1\x00", b"1e 5", b"1 e5", b"+ 1", b"nan1", b"1inf", b"-", b"..", b"1.e", b"e", b"E", b"\xef\xbc\x91", b"1e\xef\xbc\x91")]
SYNTAX += [(t, True) for t in (
    b"0", b"1", b"-1", b"+1", b"01", b"1.0", b".0", b"0.0", b"00.00", b"1e0", b"1E0", b"1e+0", b"1e-0", b"1e0000", b"1e9999", b"1e-9999", b".5e1", b"5.5e+01",
    b"inf", b"Inf", b"iNF", b"nan", b"NAN", b"-nan", b"+inf", b"12345678901234567", b"0.12345678901234567", b"1234567890.1234567e-300", b"0e99",
    b"123456789012345678", b"1.00000000000000001")]


_CACHE = {}


def rule(key, texts):
    """[bam.float_from_text(t)] of a list of texts, made once per process and key (the tests share it and leave it unchanged)"""
    from ribodetector_amd import bam
    if key not in _CACHE:
        _CACHE[key] = [bam.float_from_text(t) for t in texts]
    assert len(_CACHE[key]) == len(texts)
    return _CACHE[key]


def _value(b):
    """the exact value of a pattern in [0, INF], INF standing for 2^128"""
    return Fraction(2) ** 128 if b == INF else F.value_of(b)


def by_fractions(M, q, negative=False):
    """the pattern nearest to M 10^q (M > 0) by exact comparison of Fractions: the largest pattern at or below the value by bisection
    over the patterns - which are ordered as their values are -, then the nearer of it and the next, the even one on a tie; a value at
    or above 2^128 - 2^103 is infinity. It knows nothing of exponents, ulps or denormals."""
    v = Fraction(M) * Fraction(10) ** q
    lo, hi = 0, INF
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _value(mid) <= v:
            lo = mid
        else:
            hi = mid - 1
    b = lo
    if b < INF:
        below, above = v - _value(b), _value(b + 1) - v
        if above < below or (above == below and b & 1):
            b += 1
    return b | (SIGN if negative else 0)


def pattern_texts(patterns, fmt):
    """the texts of the finite ones among `patterns` in the form fmt ('%g', '%.9g', '%.17g'), with the patterns they came from"""
    keep = [b for b in patterns if (b >> 23) & 0xff != 0xff]
    return [g_text(b, fmt) for b in keep], keep


def random_texts(seed, n):
    """n texts (M, q, negative, text): M of 1..17 digits at exponents q = -70..45, written in a random one of the forms the syntax has -
    whole digits with an exponent, a point somewhere inside or in front of the digits, zeros in front and behind, either sign"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        s = rnd.randint(1, 17)
        M = rnd.randrange(10 ** (s - 1), 10 ** s)
        q = rnd.randint(-70, 45)
        neg = rnd.random() < 0.3
        digits = b"%d" % M
        lead, trail = (b"0" * rnd.randint(0, 3) if rnd.random() < 0.2 else b""), (b"0" * rnd.randint(1, 5) if rnd.random() < 0.2 else b"")
        form = rnd.randrange(4)
        if form == 0:                                      # whole digits
            mant, x = lead + digits + trail, q - len(trail)
        elif form == 1:                                    # a point inside (or behind the first digit)
            cut = rnd.randint(1, len(digits))
            frac = digits[cut:] + trail
            mant, x = (lead + digits[:cut] + b"." + frac, q + len(digits) - cut) if frac else (lead + digits[:cut], q)
        elif form == 2:                                    # .ddd
            mant, x = lead + b"." + digits + trail, q + len(digits)
        else:                                              # 0.000ddd
            z = rnd.randint(1, 6)
            mant, x = b"0." + b"0" * z + digits + trail, q + len(digits) + z
        expo = b"" if x == 0 and rnd.random() < 0.5 else (b"e" if rnd.random() < 0.8 else b"E") + (b"+" if x >= 0 and rnd.random() < 0.3 else b"") + b"%d" % x
        out.append((M, q, neg, (b"-" if neg else b"+" if rnd.random() < 0.05 else b"") + mant + expo))
    return out


def midpoint_texts(seed, per_exponent):
    """[(text, want)] around the midpoints (2 m + 1) 2^(e - 1) between two neighbouring floats m 2^e and (m + 1) 2^e: for every exponent
    field (denormals included) the mantissas 0, 1, 2^23 - 2, 2^23 - 1 and per_exponent random ones. A midpoint's exact decimal has
    finitely many digits; with at most 17 of them (e - 1 between about -11 and 26) the texts are the midpoint itself - a tie: the even
    neighbour - and its two 17-digit neighbours, one digit below and above in the 17th place; otherwise the midpoint cut to 17 digits
    and that plus one, which lie on its two sides. want is the float below or above, known from how the text was made; the midpoint
    above FLT_MAX is 2^128 - 2^103."""
    rnd = random.Random(seed)
    out = []
    for ef in range(0, 255):
        for mf in [0, 1, 2 ** 23 - 2, 2 ** 23 - 1] + [rnd.getrandbits(23) for _ in range(per_exponent)]:
            b = (ef << 23) | mf
            mid = (_value(b) + _value(b + 1)) / 2
            even = b if not b & 1 else b + 1
            N, p = _digits17(mid)
            if Fraction(N) * Fraction(10) ** p == mid:                          # at most 17 digits
                out += [(_sci(N, p), even), (_sci(N - 1, p), b), (_sci(N + 1, p), b + 1)]
                if N % 10 == 0:                                                 # at most 16: the same tie without its last zero
                    out.append((_sci(N // 10, p + 1), even))
            else:
                assert Fraction(N) * Fraction(10) ** p < mid < Fraction(N + 1) * Fraction(10) ** p
                out += [(_sci(N, p), b), (_sci(N + 1, p), b + 1)]
    return out


def exact_midpoints():
    """[(text, want)]: every midpoint whose decimal has at most 16 digits among the whole-number and half-number ones near 2^24 - the
    range in which a long-read quality or a count stands -, with its two 17-digit neighbours: (2 m + 1) 2^(e - 1) for e - 1 in -3..3 and a
    stride of mantissas"""
    out = []
    for e1 in range(-3, 4):
        for m in range(2 ** 23, 2 ** 24, 4099):
            mid = Fraction(2 * m + 1) * Fraction(2) ** e1
            b = F.exact(Fraction(m) * Fraction(2) ** (e1 + 1))
            assert b is not None
            N, p = _digits17(mid)
            assert Fraction(N) * Fraction(10) ** p == mid and N % 10 == 0
            out += [(_sci(N, p), b if not b & 1 else b + 1), (_sci(N - 1, p), b), (_sci(N + 1, p), b + 1)]
    return out
