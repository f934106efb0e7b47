"""The case table of --ubam_tags: header lines, the listed names and what bam.tags_from_comment makes of them, written out by hand
(struct, no call of the rule). tests/test_ubam_tags_host.py holds the rule against it, tests/test_gpu_ubam_tags.py the device.

A case is (what it shows, header line, names, tag bytes or None for a malformed record, copied per name, float values skipped)."""
import struct

MM_ML_RG = [b"MM", b"ML", b"RG"]
XI = [b"XI"]


def _i(name, v):
    """a scalar integer in the smallest type"""
    if v >= 0:
        t, f = (b"C", "<B") if v <= 255 else (b"S", "<H") if v <= 65535 else (b"I", "<I")
    else:
        t, f = (b"c", "<b") if v >= -128 else (b"s", "<h") if v >= -32768 else (b"i", "<i")
    return name + t + struct.pack(f, v)


def _b(name, sub, vals):
    f = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[sub]
    return name + b"B" + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), f), *vals)


CASES = [
    ("the three tags of a modified-base call", b"@r1\tMM:Z:C+m,1,2;\tML:B:C,255,0,7\tRG:Z:lib7", MM_ML_RG,
     b"MMZC+m,1,2;\0" + _b(b"ML", "C", [255, 0, 7]) + b"RGZlib7\0", [True, True, True], 0),
    ("comment order, not list order", b"@r1\tRG:Z:a\tMM:Z:b", MM_ML_RG, b"RGZa\0MMZb\0", [True, False, True], 0),
    ("an id ended by a space, an Illumina comment", b"@r1 1:N:0:ACGT", MM_ML_RG, b"", [False, False, False], 0),
    ("a space ends the id, tags behind it", b"@r1 RG:Z:x y\tMM:Z:", MM_ML_RG, b"RGZx y\0MMZ\0", [True, False, True], 0),
    ("a space inside the comment splits nothing", b"@r1\tXX:Z:1 RG:Z:no", MM_ML_RG, b"", [False, False, False], 0),
    ("CRLF: the carriage return is not part of the line", b"@r1\tRG:Z:a\r\n", MM_ML_RG, b"RGZa\0", [False, False, True], 0),
    ("CRLF without a comment", b"@r1\r\n", MM_ML_RG, b"", [False, False, False], 0),
    ("a carriage return inside the line is a byte no value holds", b"@r1\tRG:Z:a\rb\n", MM_ML_RG, None, None, 0),
    ("a carriage return ends the id", b"@r1\rRG:Z:a\n", MM_ML_RG, b"RGZa\0", [False, False, True], 0),
    ("no comment", b"@r1", MM_ML_RG, b"", [False, False, False], 0),
    ("no comment, the line's end given", b"@r1\n", MM_ML_RG, b"", [False, False, False], 0),
    ("an empty comment", b"@r1\t", MM_ML_RG, b"", [False, False, False], 0),
    ("empty fields", b"@r1\t\t\tRG:Z:q\t", MM_ML_RG, b"RGZq\0", [False, False, True], 0),
    ("an empty id", b"@\tRG:Z:q", MM_ML_RG, b"RGZq\0", [False, False, True], 0),
    ("an empty Z", b"@r1\tRG:Z:", MM_ML_RG, b"RGZ\0", [False, False, True], 0),
    ("a duplicate name: the first counts, the second is not validated", b"@r1\tRG:Z:a\tRG:i:x", MM_ML_RG, b"RGZa\0", [False, False, True], 0),
    ("a duplicate behind a malformed first", b"@r1\tRG:i:x\tRG:Z:a", MM_ML_RG, None, None, 0),
    ("an unlisted name is not validated", b"@r1\tXX:i:abc\tRG:Z:a", MM_ML_RG, b"RGZa\0", [False, False, True], 0),
    ("fields that are no tag fields", b"@r1\tRG:Z\tRG-Z:a\t1G:Z:a\tR_:Z:a\tRG:X:a\tRG:Z;a\tRG;Z:a\tRG:z:a", MM_ML_RG, b"", [False, False, False], 0),
    ("a digit as the second byte of a name", b"@r1\tX0:A:!", [b"X0"], b"X0A!", [True], 0),
    ("A", b"@r1\tXI:A:~", XI, b"XIA~", [True], 0),
    ("A: empty", b"@r1\tXI:A:", XI, None, None, 0),
    ("A: two bytes", b"@r1\tXI:A:ab", XI, None, None, 0),
    ("A: a space", b"@r1\tXI:A: ", XI, None, None, 0),
    ("A: a byte above 0x7E", b"@r1\tXI:A:\x7f", XI, None, None, 0),
    ("Z: a byte below 0x20", b"@r1\tXI:Z:a\x01b", XI, None, None, 0),
    ("Z: a byte above 0x7E", b"@r1\tXI:Z:" + b"a" * 40 + b"\x80", XI, None, None, 0),
    ("Z: every byte that may stand", b"@r1\tXI:Z:" + bytes(range(0x20, 0x7F)), XI, b"XIZ" + bytes(range(0x20, 0x7F)) + b"\0", [True], 0),
    ("H", b"@r1\tXI:H:00ffAb", XI, b"XIH00ffAb\0", [True], 0),
    ("H: empty", b"@r1\tXI:H:", XI, b"XIH\0", [True], 0),
    ("H: odd", b"@r1\tXI:H:abc", XI, None, None, 0),
    ("H: no hex digit", b"@r1\tXI:H:0g", XI, None, None, 0),
    ("H: no hex digit behind 16 good ones", b"@r1\tXI:H:" + b"0123456789abcdef" * 2 + b"zz", XI, None, None, 0),
    ("f is left out and counted", b"@r1\tXI:f:1.5\tRG:Z:a", [b"XI", b"RG"], b"RGZa\0", [False, True], 1),
    ("f is not validated", b"@r1\tXI:f:", XI, b"", [False], 1),
    ("B:f is left out and counted", b"@r1\tXI:B:f,1.5,2\tRG:Z:a", [b"XI", b"RG"], b"RGZa\0", [False, True], 1),
    ("floats of a malformed record are not counted", b"@r1\tXI:f:1\tRG:A:", [b"XI", b"RG"], None, None, 0),
    ("B: empty", b"@r1\tXI:B:", XI, None, None, 0),
    ("B: an unknown subtype", b"@r1\tXI:B:d,1", XI, None, None, 0),
    ("B: no comma behind the subtype", b"@r1\tXI:B:C1", XI, None, None, 0),
    ("B: an empty element", b"@r1\tXI:B:C,1,,2", XI, None, None, 0),
    ("B: a trailing comma", b"@r1\tXI:B:C,1,", XI, None, None, 0),
    ("B: only a comma", b"@r1\tXI:B:C,", XI, None, None, 0),
    ("B: a bad digit", b"@r1\tXI:B:C,1x", XI, None, None, 0),
    ("B: a sign inside an element", b"@r1\tXI:B:c,1-2", XI, None, None, 0),
    ("B: a space", b"@r1\tXI:B:C, 1", XI, None, None, 0),
    ("B: signs and leading zeros", b"@r1\tXI:B:s,+5,-0,007,-32768", XI, _b(b"XI", "s", [5, 0, 7, -32768]), [True], 0),
    ("B: an element of eleven digits", b"@r1\tXI:B:I,00000000001", XI, None, None, 0),
    ("16 names", b"@r1" + b"".join(b"\tX%c:i:%d" % (65 + j, j) for j in range(16)), [b"X%c" % (65 + j) for j in range(15, -1, -1)],
     b"".join(_i(b"X%c" % (65 + j), j) for j in range(16)), [True] * 16, 0),
    ("a FASTA header", b">s1 RG:Z:fa", MM_ML_RG, b"RGZfa\0", [False, False, True], 0),
]

# the integer edges: (text, value or None for malformed)
INT_EDGES = [(b"-2147483649", None), (b"-2147483648", -2147483648), (b"-32769", -32769), (b"-32768", -32768), (b"-129", -129), (b"-128", -128),
             (b"-1", -1), (b"0", 0), (b"255", 255), (b"256", 256), (b"65535", 65535), (b"65536", 65536), (b"4294967295", 4294967295),
             (b"4294967296", None), (b"+5", 5), (b"007", 7), (b"-0", 0), (b"0000000255", 255), (b"12345678901", None), (b"-", None), (b"+", None),
             (b"", None), (b"1 ", None), (b"0x1", None), (b"1.0", None), (b"--1", None)]
for _text, _v in INT_EDGES:
    CASES.append(("i: %r" % _text, b"@r1\tXI:i:" + _text, XI, None if _v is None else _i(b"XI", _v), None if _v is None else [True], 0))

# B arrays with 0 and 1 elements, and every subtype at both ends of its range and one past
B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
for _s, (_lo, _hi) in B_RANGE.items():
    CASES.append(("B:%s without elements" % _s, b"@r1\tXI:B:" + _s.encode(), XI, _b(b"XI", _s, []), [True], 0))
    CASES.append(("B:%s with one element" % _s, b"@r1\tXI:B:%s,%d" % (_s.encode(), _hi), XI, _b(b"XI", _s, [_hi]), [True], 0))
    CASES.append(("B:%s at both ends" % _s, b"@r1\tXI:B:%s,%d,%d,1" % (_s.encode(), _lo, _hi), XI, _b(b"XI", _s, [_lo, _hi, 1]), [True], 0))
    CASES.append(("B:%s below its range" % _s, b"@r1\tXI:B:%s,1,%d" % (_s.encode(), _lo - 1), XI, None, None, 0))
    CASES.append(("B:%s above its range" % _s, b"@r1\tXI:B:%s,%d,1" % (_s.encode(), _hi + 1), XI, None, None, 0))


def random_field(rnd):
    """a field of a comment: mostly a well-formed tag field of a few names, sometimes a float, no tag field at all or a malformed value"""
    kind = rnd.randrange(8)
    name = rnd.choice((b"MM", b"ML", b"RG", b"XI", b"XX"))
    if kind == 0:
        return name + b":A:" + bytes([rnd.randrange(0x21, 0x7F)])
    if kind == 1:
        return name + b":i:%d" % rnd.choice((0, 9, 255, 256, 65535, 65536, -1, -129, -40000, 2 ** 32 - 1, rnd.randrange(-2 ** 31, 2 ** 32)))
    if kind == 2:
        return name + b":Z:" + bytes(rnd.randrange(0x20, 0x7F) for _ in range(rnd.choice((0, 1, 7, 15, 16, 17, 33, 64, 100))))
    if kind == 3:
        return name + b":H:" + bytes(rnd.choice(b"0123456789abcdefABCDEF") for _ in range(2 * rnd.randrange(0, 20)))
    if kind == 4:
        sub = rnd.choice("cCsSiI")
        lo, hi = B_RANGE[sub]
        small = rnd.random() < 0.5
        return name + b":B:" + sub.encode() + b"".join(b",%d" % (rnd.randrange(max(lo, -9), min(hi, 9) + 1) if small else rnd.randrange(lo, hi + 1))
                                                     for _ in range(rnd.choice((0, 1, 2, 3, 5, 16, 17, 40))))
    if kind == 5:
        return rnd.choice((name + b":f:1.5", name + b":B:f,1,2.5", b"1:N:0:ACGT", b"", b"x", name + b":Z"))
    if kind == 6:
        return rnd.choice((name + b":i:", name + b":i:99999999999", name + b":B:C,256", name + b":B:C,1,", name + b":H:abc", name + b":A:", name + b":Z:\x7f",
                           name + b":B:q,1", name + b":B:", name + b":i:1e3"))
    return b"YY:Z:" + bytes(rnd.randrange(0x20, 0x7F) for _ in range(rnd.randrange(0, 30)))


def expected(case):
    """(tag_bytes, copied, malformed, floats) of a case, as bam.tags_from_comment returns it"""
    _, _, names, tags, copied, floats = case
    if tags is None:
        return b"", [False] * len(names), True, 0
    return tags, list(copied), False, floats
