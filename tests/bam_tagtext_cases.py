"""Hand-built BAM records for the tag comment (bam.tag_comment, C ABI rd_bam_tag_splice), shared by tests/test_bam_tagtext_host.py and
tests/test_gpu_bam_tagtext.py. A case is (name, tag bytes of the record, the tag list, want): want = the comment as a literal byte
string written by hand, or MALFORMED for a record that gets none and is counted. The records themselves come from
tests/bam_tags_cases.py's encoders."""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

MALFORMED = "malformed"
scalar, Z, B, rec = T.scalar, T.Z, T.B, T.rec


def _cases():
    out = []
    X = b"XX"
    # every scalar type at its extremes, and 0
    for t, v, text in (("c", -128, b"-128"), ("c", 127, b"127"), ("c", 0, b"0"), ("C", 255, b"255"), ("C", 0, b"0"),
                       ("s", -32768, b"-32768"), ("s", 32767, b"32767"), ("s", 0, b"0"), ("S", 65535, b"65535"), ("S", 0, b"0"),
                       ("i", -2147483648, b"-2147483648"), ("i", 2147483647, b"2147483647"), ("i", 0, b"0"),
                       ("I", 4294967295, b"4294967295"), ("I", 0, b"0"), ("i", -1, b"-1"), ("I", 1000000000, b"1000000000"), ("S", 10, b"10")):
        out.append(("scalar %s %d" % (t, v), scalar(X, t, v), [X], b"\tXX:i:" + text))
    out.append(("A", scalar(b"XA", "A", b"q"), [b"XA"], b"\tXA:A:q"))
    out.append(("A space", scalar(b"XA", "A", b" "), [b"XA"], b"\tXA:A: "))
    out.append(("A tilde", scalar(b"XA", "A", b"~"), [b"XA"], b"\tXA:A:~"))
    out.append(("A control byte", scalar(b"XA", "A", b"\x1f"), [b"XA"], MALFORMED))
    out.append(("A DEL", scalar(b"XA", "A", b"\x7f"), [b"XA"], MALFORMED))
    # every B subtype with 0, 1 and 3 elements
    for sub, one, three, t1, t3 in (("c", [-128], [127, 0, -1], b",-128", b",127,0,-1"), ("C", [255], [0, 9, 100], b",255", b",0,9,100"),
                                    ("s", [-32768], [32767, -1, 10], b",-32768", b",32767,-1,10"), ("S", [65535], [0, 99, 1000], b",65535", b",0,99,1000"),
                                    ("i", [-2147483648], [2147483647, 0, -10], b",-2147483648", b",2147483647,0,-10"),
                                    ("I", [4294967295], [0, 1, 99999], b",4294967295", b",0,1,99999")):
        head = b"\tML:B:" + sub.encode()
        out.append(("B:%s of 0" % sub, B(b"ML", sub, []), [b"ML"], head))
        out.append(("B:%s of 1" % sub, B(b"ML", sub, one), [b"ML"], head + t1))
        out.append(("B:%s of 3" % sub, B(b"ML", sub, three), [b"ML"], head + t3))
    out.append(("Z empty", Z(b"MM", b""), [b"MM"], b"\tMM:Z:"))
    out.append(("Z", Z(b"MM", b"C+m,5,12,0;"), [b"MM"], b"\tMM:Z:C+m,5,12,0;"))
    out.append(("Z with spaces", Z(b"CO", b"a b  c~"), [b"CO"], b"\tCO:Z:a b  c~"))
    out.append(("H", Z(b"XH", b"1AE30f", "H"), [b"XH"], b"\tXH:H:1AE30f"))
    out.append(("H empty", Z(b"XH", b"", "H"), [b"XH"], b"\tXH:H:"))
    out.append(("H of odd length", Z(b"XH", b"1AE", "H"), [b"XH"], MALFORMED))
    out.append(("H with a non-hex character", Z(b"XH", b"1AG3", "H"), [b"XH"], MALFORMED))
    # tag-level behaviour
    three = Z(b"RG", b"grp1") + scalar(b"NM", "i", 7) + B(b"ML", "C", [1, 22, 255])
    out.append(("list order, not record order", three, [b"ML", b"RG", b"NM"], b"\tML:B:C,1,22,255\tRG:Z:grp1\tNM:i:7"))
    out.append(("record order when the list says so", three, [b"RG", b"NM", b"ML"], b"\tRG:Z:grp1\tNM:i:7\tML:B:C,1,22,255"))
    out.append(("the first of two wins", Z(b"RG", b"one") + scalar(b"NM", "i", 1) + Z(b"RG", b"second"), [b"RG"], b"\tRG:Z:one"))
    out.append(("an absent tag", three, [b"MM", b"RG"], b"\tRG:Z:grp1"))
    out.append(("no listed tag present", three, [b"MM", b"XY"], b""))
    out.append(("no tags at all", b"", [b"RG"], b""))
    out.append(("f skipped, the others kept", scalar(b"qs", "f", 12.5) + Z(b"RG", b"a"), [b"qs", b"RG"], b"\tRG:Z:a"))
    out.append(("B:f skipped, the others kept", Z(b"RG", b"a") + B(b"XF", "f", [0.5, 2.0]) + scalar(b"NM", "C", 3), [b"RG", b"XF", b"NM"],
                b"\tRG:Z:a\tNM:i:3"))
    out.append(("f not listed is not counted", scalar(b"qs", "f", 12.5) + Z(b"RG", b"a"), [b"RG"], b"\tRG:Z:a"))
    out.append(("a malformed tag in front of a listed one", scalar(b"NM", "i", 7) + b"XQq\x01\x02\x03\x04" + Z(b"RG", b"a"), [b"NM", b"RG"], MALFORMED))
    out.append(("a malformed tag behind all listed ones", Z(b"RG", b"a") + scalar(b"NM", "i", 7) + b"XQq\x01", [b"NM", b"RG"], b"\tNM:i:7\tRG:Z:a"))
    out.append(("a listed tag that is absent, in front of the damage", Z(b"RG", b"a") + b"XQq\x01", [b"RG", b"MM"], MALFORMED))
    out.append(("a control byte in Z", Z(b"RG", b"a\x01b"), [b"RG"], MALFORMED))
    out.append(("a tab in Z", Z(b"RG", b"a\tb"), [b"RG"], MALFORMED))
    out.append(("a newline in Z", Z(b"RG", b"a\nb"), [b"RG"], MALFORMED))
    out.append(("a byte above 0x7E in Z", Z(b"RG", b"a\x80b"), [b"RG"], MALFORMED))
    out.append(("a newline in a Z that is not listed", Z(b"CO", b"a\nb") + Z(b"RG", b"g"), [b"RG"], b"\tRG:Z:g"))
    out.append(("a newline at byte 40 of a long Z", Z(b"RG", b"x" * 40 + b"\n" + b"y" * 30), [b"RG"], MALFORMED))
    out.append(("Z without a NUL", scalar(b"NM", "i", 7) + b"RGZabc", [b"NM", b"RG"], MALFORMED))
    return out


CASES = _cases()
FLOATS = {"f skipped, the others kept": 1, "B:f skipped, the others kept": 1}       # float values a case skips (every other one: 0)


def case_record(k, tags, **kw):
    return rec(tags, name=b"case%d" % k, **kw)


def digits_values(sub):
    """values of subtype `sub` of every digit count, its extremes included"""
    lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-2 ** 15, 2 ** 15 - 1), "S": (0, 2 ** 16 - 1), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}[sub]
    vals = [lo, hi, 0]
    p = 1
    while p <= hi:
        vals += [p, min(hi, 10 * p - 1)]
        if -p >= lo:
            vals += [-p, max(lo, -(10 * p - 1))]
        p *= 10
    return vals


def b_values(sub, count, seed=0):
    base = digits_values(sub)
    rnd = random.Random(seed * 1000 + count)
    return [base[(i + rnd.randrange(3)) % len(base)] for i in range(count)]


def random_records(seed, n, malformed=0.1):
    """(records, tag list): n records with random tag lists over all types (floats included), a share `malformed` of them damaged in
    the ways find_tag lists (cut tags, an unknown type, a Z without NUL, a B that overruns) or carrying a byte no header line may hold"""
    rnd = random.Random(seed)
    names = [b"MM", b"ML", b"RG", b"NM", b"XA", b"XH", b"qs", b"XF", b"XS"]
    out = []
    for k in range(n):
        tags = []
        for name in rnd.sample(names, rnd.randrange(0, len(names) + 1)):
            kind = rnd.randrange(7)
            if kind == 0:
                t = rnd.choice("cCsSiI")
                tags.append(scalar(name, t, rnd.choice(digits_values(t))))
            elif kind == 1:
                tags.append(Z(name, bytes(rnd.randrange(32, 127) for _ in range(rnd.choice((0, 1, 5, 15, 16, 17, 40, 130))))))
            elif kind == 2:
                sub = rnd.choice("cCsSiI")
                tags.append(B(name, sub, [rnd.choice(digits_values(sub)) for _ in range(rnd.choice((0, 1, 3, 17, 70)))]))
            elif kind == 3:
                tags.append(scalar(name, "A", bytes([rnd.randrange(32, 127)])))
            elif kind == 4:
                tags.append(Z(name, bytes(rnd.choice(b"0123456789abcdefABCDEF") for _ in range(2 * rnd.randrange(0, 20))), "H"))
            elif kind == 5:
                tags.append(scalar(name, "f", rnd.random()))
            else:
                tags.append(B(name, "f", [rnd.random() for _ in range(rnd.randrange(0, 5))]))
        tags = b"".join(tags)
        if rnd.random() < malformed:
            how = rnd.randrange(6)
            if how == 0 and tags:
                tags = tags[:rnd.randrange(len(tags))]
            elif how == 1:
                tags = b"XQq\x01\x02" + tags
            elif how == 2:
                tags = tags + b"RGZnonul"
            elif how == 3:
                tags = b"MLBC" + struct.pack("<I", 1000) + b"\x01\x02" + tags
            elif how == 4:
                tags = Z(b"RG", b"a\nb") + tags
            else:
                tags = Z(b"XH", b"abc", "H") + tags
        seq = "".join(rnd.choice("ACGTN") for _ in range(rnd.randrange(0, 60)))
        flag = rnd.choice((4, 4, 4, 0x10, 0x14))
        out.append(rec(tags, name=b"read%d" % k, seq=seq, flag=flag))
    return out, [b"RG", b"MM", b"ML", b"NM", b"XA", b"XH", b"qs", b"XF"]


def file_data(records, text=b""):
    """the inflated bytes of a BAM file of these records (bam.fastq_text_tagged and bam.records take them)"""
    return bam.encode_header((), text) + b"".join(records)
