"""float32 bit patterns for the %g text of float BAM tags (bam.float_g, C ABI rd_float_text / rd_bam_tag_splice_ex), shared by
tests/test_bam_floats_host.py, tests/test_float_text_host.py and tests/test_gpu_bam_floats.py. Everything here is a bit pattern (an int
below 2^32): a NaN's payload and a zero's sign do not survive a trip through a Python float. The records come from the encoders of
tests/bam_tags_cases.py; f_tag / bf_tag write a float tag from bit patterns."""
import os
import random
import struct
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tags_cases as T  # noqa: E402

FLT_MIN, FLT_MAX, DENORM_MIN, DENORM_MAX = 0x00800000, 0x7f7fffff, 0x00000001, 0x007fffff
INF, SIGN = 0x7f800000, 0x80000000
NANS = [0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa00000, 0xffc12345]


def bits_of(x):
    """the bit pattern of the float32 nearest to the number x (a float, an int or a Fraction; ties to even)"""
    return struct.unpack("<I", struct.pack("<f", float(x) if not isinstance(x, Fraction) else x.numerator / x.denominator))[0]


def value_of(bits):
    """the exact value of a finite pattern, as a Fraction"""
    ef, mf = (bits >> 23) & 0xff, bits & 0x7fffff
    assert ef != 0xff
    m, e = (mf | 0x800000, ef - 150) if ef else (mf, -149)
    v = Fraction(m) * Fraction(2) ** e
    return -v if bits >> 31 else v


def exact(x):
    """the pattern of the number x if a float32 holds it exactly, else None"""
    x = Fraction(x)
    try:
        b = bits_of(x)
    except OverflowError:
        return None
    return b if (b & 0x7fffffff) < INF and value_of(b) == x else None


def neighbours(bits):
    """the patterns next to a positive finite one, below and above"""
    return [b for b in (bits - 1, bits + 1) if 0 <= b <= FLT_MAX]


def _whole(values):
    """the patterns of whole numbers that a float32 holds exactly (checked)"""
    v = np.asarray(values, dtype=np.int64)
    f = v.astype(np.float32)
    assert (f.astype(np.int64) == v).all()
    return f.view(np.uint32).tolist()


def ties():
    """every exact tie of the rounding to 6 digits, found by search: {name: [patterns]}"""
    out = {}
    # whole numbers n in [10^6, 2^24] that end in 5 (every one is a float): with 7 digits the 5 is the 7th, an exact half
    out["n5"] = _whole(np.arange(10 ** 6 + 5, 2 ** 24 + 1, 10))
    # above 2^24: v = (10 q + 5) 10^j with 6 digits q and j >= 1 zeros behind the 5 is (2 q + 1) 5^(j + 1) 2^j, a float when the odd
    # part stays below 2^24 - which leaves j = 1
    big = []
    for j in range(1, 32):
        q = np.arange(10 ** 5, 10 ** 6, dtype=np.int64)
        q = q[(2 * q + 1) * 5 ** (j + 1) < 2 ** 24]
        if not len(q):
            break
        v = (10 * q + 5) * 10 ** j
        big += _whole(v[v > 2 ** 24])
    out["big"] = big
    # k + 0.5 for k of 6 digits (below 2^20 a float has the half bit): sampled, both parities
    rnd = random.Random(5)
    ks = [100000, 100001, 999998, 999999] + [rnd.randrange(100000, 1000000) for _ in range(3000)]
    assert len([k for k in ks if k & 1]) > 1000 and len([k for k in ks if not k & 1]) > 1000
    out["half"] = [exact(Fraction(2 * k + 1, 2)) for k in ks]
    assert all(b is not None for b in out["half"])
    return out


_HARD = []


def hard():
    """the patterns at which a formatter goes wrong (made once per process). Both signs of each, but for the two large families of
    ties (1.7 million whole numbers), which stand with the positive sign only: the sign is one bit that the digits do not see, and
    every other family carries it."""
    if _HARD:
        return _HARD[0]
    pos = [0, INF, DENORM_MIN, DENORM_MAX, FLT_MIN, FLT_MAX]
    pos += [exact(Fraction(2) ** e) for e in range(-149, 128)]
    for p in range(-45, 39):                               # the powers of ten: exact ones (10^0 .. 10^10) and the floats around the others
        b = bits_of(Fraction(10) ** p)
        pos += [b] + neighbours(b)
    for p in (-5, -4, 5, 6, 7):                            # where the notation changes: the floats nearest below and above
        b = bits_of(Fraction(10) ** p)
        pos += [b - 2, b - 1, b, b + 1, b + 2]
    for p in range(-10, 11):                               # 9.999995 10^p: the carry of all nines, and the floats around it
        b = bits_of(Fraction(9999995, 10 ** 6) * Fraction(10) ** p)
        pos += [b - 2, b - 1, b, b + 1, b + 2]
        b = bits_of(Fraction(99999949, 10 ** 7) * Fraction(10) ** p)
        pos += [b - 1, b, b + 1]
    t = ties()
    pos += t["half"] + [exact(Fraction(v)) & ~SIGN for v, _ in TIE_LITERALS]
    assert all(b is not None and 0 <= b <= INF for b in pos)
    _HARD.append([b for p in pos for b in (p, p | SIGN)] + list(NANS) + t["n5"] + t["big"])
    return _HARD[0]


_RULE = {}


def rule_texts(key, patterns):
    """[bam.float_g(b)] of a list of patterns, made once per process and key (the tests share it and leave it unchanged)"""
    from ribodetector_amd import bam
    if key not in _RULE:
        _RULE[key] = [bam.float_g(b) for b in patterns]
    assert len(_RULE[key]) == len(patterns)
    return _RULE[key]


def sweep(seed, n):
    """for every one of the 256 exponent fields: the mantissas 0, 1, 2^23 - 1, 2^22, and n random ones, both signs"""
    rnd = random.Random(seed)
    out = []
    for ef in range(256):
        for mf in [0, 1, 2 ** 23 - 1, 2 ** 22] + [rnd.getrandbits(23) for _ in range(n)]:
            out.append((rnd.getrandbits(1) << 31) | (ef << 23) | mf)
            out.append(((ef << 23) | mf) ^ (out[-1] & SIGN) ^ SIGN)
    return out


def randoms(seed, n):
    rnd = random.Random(seed)
    return [rnd.getrandbits(32) for _ in range(n)]


def f_tag(name, bits, size=4):
    """an f tag from a bit pattern (size < 4: a value cut short - the record ends in it)"""
    return name + b"f" + struct.pack("<I", bits)[:size]


def bf_tag(name, patterns):
    return name + b"Bf" + struct.pack("<I", len(patterns)) + struct.pack("<%dI" % len(patterns), *patterns)


# hand-written: (a number that a float32 holds exactly, as decimal text; what %g prints). Each is an exact tie: it goes to the even digit.
TIE_LITERALS = [
    ("100000.5", b"100000"), ("100001.5", b"100002"), ("100002.5", b"100002"), ("999999.5", b"1e+06"), ("999998.5", b"999998"),
    ("123456.5", b"123456"), ("123457.5", b"123458"), ("1234565", b"1.23456e+06"), ("1234575", b"1.23458e+06"), ("1000005", b"1e+06"),
    ("1000015", b"1.00002e+06"), ("9999995", b"1e+07"), ("16777150", b"1.67772e+07"), ("16777250", b"1.67772e+07"),
    ("33554350", b"3.35544e+07"), ("-100001.5", b"-100002"),
]
# hand-written: (the number whose nearest float32 is meant; what %g prints)
LITERALS = [
    ("12.5", b"12.5"), ("0.0001", b"0.0001"), ("0.00001", b"1e-05"), ("100000", b"100000"), ("1000000", b"1e+06"), ("0.5", b"0.5"), ("-2", b"-2"),
    ("3.5", b"3.5"), ("0.25", b"0.25"), ("1024", b"1024"), ("65536", b"65536"), ("1048576", b"1.04858e+06"), ("0.1", b"0.1"), ("1e10", b"1e+10"),
    ("3.4028234663852886e38", b"3.40282e+38"), ("1.401298464324817e-45", b"1.4013e-45"), ("1.1754943508222875e-38", b"1.17549e-38"),
    ("123456789", b"1.23457e+08"), ("0.000123456789", b"0.000123457"), ("99999.95", b"100000"), ("99999.94", b"99999.9"), ("999999.4", b"999999"),
]


def tagged_cases():
    """(name, tag bytes, tag list, comment with floats on, comment without) - the float cases of the tag comment, literals by hand"""
    h = bits_of
    Z, sc = T.Z, T.scalar
    return [
        ("qs:f 12.5", f_tag(b"qs", h(12.5)), [b"qs"], b"\tqs:f:12.5", b""),
        ("f -0", f_tag(b"qs", SIGN), [b"qs"], b"\tqs:f:-0", b""),
        ("f nan with its sign", f_tag(b"qs", 0xffc00000), [b"qs"], b"\tqs:f:-nan", b""),
        ("f inf", f_tag(b"qs", INF), [b"qs"], b"\tqs:f:inf", b""),
        ("f the longest text", f_tag(b"qs", FLT_MIN | SIGN), [b"qs"], b"\tqs:f:-1.17549e-38", b""),
        ("f a tie", f_tag(b"rq", h(100001.5)), [b"rq"], b"\trq:f:100002", b""),
        ("B:f of 0", bf_tag(b"XF", []), [b"XF"], b"\tXF:B:f", b""),
        ("B:f of 1", bf_tag(b"XF", [h(0.5)]), [b"XF"], b"\tXF:B:f,0.5", b""),
        ("B:f of 3", bf_tag(b"XF", [h(0.5), h(2.0), h(-1e10)]), [b"XF"], b"\tXF:B:f,0.5,2,-1e+10", b""),
        ("f between two integers, list order", sc(b"NM", "i", 7) + f_tag(b"qs", h(9.75)) + sc(b"XS", "C", 3), [b"XS", b"qs", b"NM"],
         b"\tXS:i:3\tqs:f:9.75\tNM:i:7", b"\tXS:i:3\tNM:i:7"),
        ("B:f between Z and B:C", Z(b"RG", b"a") + bf_tag(b"XF", [h(1.5), h(1e-5)]) + T.B(b"ML", "C", [1, 2]), [b"RG", b"XF", b"ML"],
         b"\tRG:Z:a\tXF:B:f,1.5,1e-05\tML:B:C,1,2", b"\tRG:Z:a\tML:B:C,1,2"),
        ("the first of two f wins", f_tag(b"qs", h(1.0)) + f_tag(b"qs", h(2.0)), [b"qs"], b"\tqs:f:1", b""),
        ("f not listed", f_tag(b"qs", h(12.5)) + Z(b"RG", b"a"), [b"RG"], b"\tRG:Z:a", b"\tRG:Z:a"),
    ]


# records whose float tag cannot be walked: malformed with floats on and off (the walk decides it)
MALFORMED_CASES = [
    ("f cut to 3 bytes", T.scalar(b"NM", "i", 7) + f_tag(b"qs", 0x41480000, size=3), [b"NM", b"qs"]),
    ("B:f that overruns", T.Z(b"RG", b"a") + b"XFBf" + struct.pack("<I", 3) + struct.pack("<2I", 1, 2), [b"RG", b"XF"]),
]
