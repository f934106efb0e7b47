"""The case table of --ubam_tag_floats: comments, the listed names and what bam.tags_from_comment(floats=True) makes of them, written out
by hand (struct and bit patterns, no call of the rule). tests/test_ubam_tag_floats_host.py holds the rule against it,
tests/test_gpu_ubam_tag_floats.py the device.

A case is (what it shows, the comment behind '@r1<TAB>', names, tag bytes or None for a malformed record, (copied per name, float
values skipped))."""
import struct

QS, XF = [b"qs"], [b"XF"]
LONG = b"1.00000005960464478"        # 18 significant digits: not converted


def f(name, bits):
    return name + b"f" + struct.pack("<I", bits)


def bf(name, patterns):
    return name + b"Bf" + struct.pack("<I%dI" % len(patterns), len(patterns), *patterns)


def _bad(what, comment, names):
    return (what, comment, names, None, None)


CASES = [
    ("qs:f of a basecaller", b"qs:f:12.5", QS, f(b"qs", 0x41480000), ([True], 0)),
    ("f -0 keeps its sign", b"qs:f:-0", QS, f(b"qs", 0x80000000), ([True], 0)),
    ("f -nan keeps its sign, not its payload", b"qs:f:-nan", QS, f(b"qs", 0xffc00000), ([True], 0)),
    ("f inf, any letter case", b"qs:f:+INF", QS, f(b"qs", 0x7f800000), ([True], 0)),
    ("f the longest %g text", b"qs:f:-1.17549e-38", QS, f(b"qs", 0x807fffe1), ([True], 0)),
    ("f a tie goes to the even mantissa", b"qs:f:16777217", QS, f(b"qs", 0x4b800000), ([True], 0)),
    ("f without digits in front of the point", b"qs:f:.5", QS, f(b"qs", 0x3f000000), ([True], 0)),
    ("f 17 digits", b"qs:f:1.0000000596046448", QS, f(b"qs", 0x3f800001), ([True], 0)),
    ("f overflow is infinity", b"qs:f:1e9999", QS, f(b"qs", 0x7f800000), ([True], 0)),
    ("f underflow is zero", b"qs:f:-1e-9999", QS, f(b"qs", 0x80000000), ([True], 0)),
    ("f the smallest denormal", b"qs:f:1.4013e-45", QS, f(b"qs", 0x00000001), ([True], 0)),
    ("f empty", b"qs:f:", QS, None, None),
    ("f a point without a fraction", b"qs:f:5.", QS, None, None),
    ("f an exponent without digits", b"qs:f:1e", QS, None, None),
    ("f five exponent digits", b"qs:f:1e12345", QS, None, None),
    ("f a hex float", b"qs:f:0x1p3", QS, None, None),
    ("f infinity spelled out", b"qs:f:infinity", QS, None, None),
    ("f a space", b"qs:f:1 ", QS, None, None),
    ("f a comma", b"qs:f:1,2", QS, None, None),
    ("f 18 digits: left out and counted", b"qs:f:" + LONG, QS, b"", ([False], 1)),
    ("f 18 digits between two other tags: they stay", b"RG:Z:a\tqs:f:" + LONG + b"\tNM:i:7", [b"qs", b"RG", b"NM"], b"RGZa\0NMC\x07", ([False, True, True], 1)),
    ("B:f without elements", b"XF:B:f", XF, bf(b"XF", []), ([True], 0)),
    ("B:f of 1", b"XF:B:f,0.5", XF, bf(b"XF", [0x3f000000]), ([True], 0)),
    ("B:f of 3", b"XF:B:f,0.5,2,-1e+10", XF, bf(b"XF", [0x3f000000, 0x40000000, 0xd01502f9]), ([True], 0)),
    ("B:f specials", b"XF:B:f,nan,-inf,-0,1e-46", XF, bf(b"XF", [0x7fc00000, 0xff800000, 0x80000000, 0]), ([True], 0)),
    ("B:f an empty element", b"XF:B:f,1,,2", XF, None, None),
    ("B:f a trailing comma", b"XF:B:f,1,", XF, None, None),
    ("B:f only a comma", b"XF:B:f,", XF, None, None),
    ("B:f no comma behind the subtype", b"XF:B:f1", XF, None, None),
    ("B:f an element that is no number", b"XF:B:f,1,x,2", XF, None, None),
    ("B:f an element that ends early", b"XF:B:f,1,2.,3", XF, None, None),
    ("B:f a skipped element in a good array: the whole tag is left out, once", b"XF:B:f,1," + LONG + b",2," + LONG, XF, b"", ([False], 1)),
    ("B:f a skipped and a malformed element: malformed", b"XF:B:f," + LONG + b",x", XF, None, None),
    ("B:f a malformed and a skipped element: malformed", b"XF:B:f,x," + LONG, XF, None, None),
    ("the float first", b"qs:f:9.75\tNM:i:7\tRG:Z:a", [b"RG", b"qs", b"NM"], f(b"qs", 0x411c0000) + b"NMC\x07RGZa\0", ([True, True, True], 0)),
    ("the float last", b"NM:i:7\tRG:Z:a\tqs:f:9.75", [b"RG", b"qs", b"NM"], b"NMC\x07RGZa\0" + f(b"qs", 0x411c0000), ([True, True, True], 0)),
    ("B:f between Z and B:C", b"RG:Z:a\tXF:B:f,1.5,1e-05\tML:B:C,1,2", [b"RG", b"XF", b"ML"],
     b"RGZa\0" + bf(b"XF", [0x3fc00000, 0x3727c5ac]) + b"MLBC\x02\0\0\0\x01\x02", ([True, True, True], 0)),
    ("a float in a malformed record counts nothing", b"qs:f:1.5\tRG:A:", [b"qs", b"RG"], None, None),
    ("a skipped float in a malformed record counts nothing", b"qs:f:" + LONG + b"\tRG:A:", [b"qs", b"RG"], None, None),
    ("a malformed float behind good tags: no tags at all", b"RG:Z:a\tqs:f:1e", [b"qs", b"RG"], None, None),
    ("the first of two f counts, the second is not validated", b"qs:f:1\tqs:f:x", QS, f(b"qs", 0x3f800000), ([True], 0)),
    ("a duplicate behind a malformed first", b"qs:f:x\tqs:f:1", QS, None, None),
    ("a duplicate behind a skipped first stays out", b"qs:f:" + LONG + b"\tqs:f:1", QS, b"", ([False], 1)),
    ("f not listed is not validated", b"qs:f:x\tRG:Z:a", [b"RG"], b"RGZa\0", ([True], 0)),
    ("two skipped tags count two", b"qs:f:" + LONG + b"\tXF:B:f," + LONG, [b"qs", b"XF"], b"", ([False, False], 2)),
]


def header(comment, k=1):
    return b"@r%d\t" % k + comment


def expected(case):
    """(tag_bytes, copied, malformed, floats) of a case, as bam.tags_from_comment(floats=True) returns it"""
    _, _, names, tags, counts = case
    if tags is None:
        return b"", [False] * len(names), True, 0
    return tags, list(counts[0]), False, counts[1]


def fastq(records):
    """FASTQ text of (name, comment) pairs with four bases each"""
    return b"".join(b"@" + n + b"\t" + c + b"\nACGT\n+\nIIII\n" for n, c in records)
