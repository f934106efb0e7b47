"""Hand-built BAM records for the tag walk (bam.find_tag, C ABI rd_bam_tag_find), shared by tests/test_bam_tags_host.py and
tests/test_gpu_bam_tags.py. A case is (name, record bytes, want): want = ("found", value bytes, type letter) / "none" / "malformed" for
the tag RG - what the construction says, stated without running the walk. CASES keeps the ORDER of the records: the overrun decoys
depend on the record that follows them in a raw view."""
import random
import struct

from ribodetector_amd import bam

TARGET = b"RG"
_FMT = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
_B_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


def scalar(name, t, value):
    return name + t.encode() + struct.pack(_FMT[t], value)


def Z(name, value, t="Z"):
    return name + t.encode() + bytes(value) + b"\0"


def B(name, sub, values):
    return name + b"B" + sub.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), _B_FMT[sub]), *values)


def rec(tags, name=b"r", seq="ACGTACGTAC", **kw):
    return bam.encode_record(dict({"name": name, "seq": seq, "qual": bytes(len(seq)), "tags": tags}, **kw))


def _cases():
    out = []
    rg = Z(TARGET, b"grp1")
    found = ("found", b"grp1", "Z")
    small = scalar(b"NM", "i", 7) + scalar(b"XA", "A", b"q")
    # every scalar type as the target and in front of it; B with every subtype, and with no elements
    for t, v in (("A", b"x"), ("c", -5), ("C", 250), ("s", -300), ("S", 65000), ("i", -70000), ("I", 4000000000), ("f", 1.5)):
        out.append(("scalar %s is the target" % t, rec(scalar(TARGET, t, v)), ("found", struct.pack(_FMT[t], v), t)))
        out.append(("scalar %s in front" % t, rec(scalar(b"X" + t.encode(), t, v) + rg), found))
    for sub, vals in (("c", [-1, 2, 3]), ("C", [1, 2, 255]), ("s", [-2, 5]), ("S", [7, 65535, 9]), ("i", [-9]), ("I", [1, 2]), ("f", [0.5, 2.0, 3.0])):
        arr = B(b"ML", sub, vals)
        out.append(("B:%s in front" % sub, rec(arr + rg), found))
        out.append(("B:%s is the target" % sub, rec(B(TARGET, sub, vals) + small), ("found", arr[3:], "B")))
        out.append(("B:%s of no elements in front" % sub, rec(B(b"ML", sub, []) + rg), found))
    out.append(("B of no elements is the target, last", rec(small + B(TARGET, "C", [])), ("found", b"C\0\0\0\0", "B")))
    # where the target stands
    out.append(("target first", rec(rg + small), found))
    out.append(("target in the middle", rec(small + rg + Z(b"BC", b"ACGT")), found))
    out.append(("target last", rec(small + Z(b"BC", b"ACGT") + rg), found))
    out.append(("target absent", rec(small + Z(b"BC", b"ACGT")), "none"))
    out.append(("no tags", rec(b""), "none"))
    out.append(("the first of two wins", rec(Z(TARGET, b"one") + small + Z(TARGET, b"second")), ("found", b"one", "Z")))
    out.append(("Z of no bytes is the target", rec(Z(TARGET, b"")), ("found", b"", "Z")))
    out.append(("Z of no bytes in front", rec(Z(b"XZ", b"") + rg), found))
    out.append(("H in front", rec(Z(b"XH", b"1AE3", "H") + rg), found))
    out.append(("H is the target", rec(Z(TARGET, b"1AE3", "H")), ("found", b"1AE3", "H")))
    out.append(("RG:i", rec(scalar(TARGET, "i", 3)), ("found", struct.pack("<i", 3), "i")))
    for n in (15, 16, 17, 63, 64, 65, 4097):           # the NUL search across its step boundaries
        val = bytes(65 + (i * 7) % 26 for i in range(n))
        out.append(("Z of %d bytes in front" % n, rec(Z(b"MM", val) + rg), found))
        out.append(("Z of %d bytes is the target" % n, rec(small + Z(TARGET, val)), ("found", val, "Z")))
        out.append(("Z of %d bytes and nothing behind" % n, rec(Z(b"MM", val)), "none"))
    out.append(("the NUL is the record's last byte, target found", rec(small + rg), found))
    out.append(("the NUL is the record's last byte, target absent", rec(small + Z(b"BC", b"AC")), "none"))
    # the fixed part in front of the tags
    out.append(("l_seq 0", rec(rg, seq=""), found))
    out.append(("l_seq 1", rec(rg, seq="A"), found))
    out.append(("odd l_seq", rec(small + rg, seq="ACGTACG"), found))
    out.append(("cigar", rec(small + rg, cigar=[(4, "S"), (5, "M"), (1, "I")], pos=100, ref_id=0, flag=0), found))
    out.append(("a name of 254 bytes", rec(small + rg, name=b"n" * 254), found))
    # malformed tags
    out.append(("1 byte left, target absent", rec(small + b"R"), "malformed"))
    out.append(("2 bytes left, target absent", rec(small + TARGET), "malformed"))
    out.append(("1 byte left behind the target", rec(rg + b"R"), found))
    out.append(("unknown type", rec(small + b"XQq\x01\x02\x03\x04" + rg), "malformed"))
    out.append(("unknown type of the target", rec(TARGET + b"z" + b"abc\0"), "malformed"))
    out.append(("unknown B subtype", rec(b"MLBd" + struct.pack("<I", 1) + b"\x01" + rg), "malformed"))
    out.append(("B of 2^32 - 1 elements", rec(b"MLBC" + struct.pack("<I", 0xFFFFFFFF) + b"\x01\x02" + rg), "malformed"))
    out.append(("B of 2^32 - 1 four-byte elements", rec(b"MLBI" + struct.pack("<I", 0xFFFFFFFF) + rg), "malformed"))
    out.append(("B one byte too long", rec(b"MLBs" + struct.pack("<I", 3) + b"\x01\x02\x03\x04\x05"), "malformed"))
    out.append(("B that ends with the record", rec(b"MLBs" + struct.pack("<I", 3) + b"\x01\x02\x03\x04\x05\x06"), "none"))
    out.append(("B whose head is cut", rec(small + b"MLBC\x01\x00"), "malformed"))
    out.append(("Z without a NUL", rec(small + b"BCZACGTACGTACGTACGTACGTA"), "malformed"))
    out.append(("Z without a byte", rec(small + b"BCZ"), "malformed"))
    out.append(("target Z without a NUL", rec(TARGET + b"Zgrp1"), "malformed"))
    out.append(("the target's scalar is cut", rec(small + TARGET + b"i\x01\x02"), "malformed"))
    out.append(("a scalar in front is cut", rec(b"NMi\x01\x02\x03"), "malformed"))
    # the overrun decoys: a walk that does not stop at the record's end finds RG:Z in the bytes of the NEXT record
    # (a) 2 stray bytes "RG"; the next record's block_size is 0x5A = 'Z' followed by three NULs: an unbounded walk reads RG:Z:""
    nxt = rec(Z(b"XY", b"v" * 37), name=b"d", seq="ACGTACGTAC")
    assert nxt[:4] == b"Z\0\0\0"
    out.append(("decoy: stray RG, then a record that starts with Z NUL", rec(small + TARGET), "malformed"))
    out.append(("decoy: the record behind it", nxt, "none"))
    # (b) Z without a NUL; the NUL search would run into the next record, whose first tag is RG
    out.append(("decoy: Z without a NUL, then a record with RG", rec(b"BCZAC"), "malformed"))
    out.append(("decoy: the record behind it", rec(rg, seq=""), found))
    # (c) no tags; the bytes behind the record spell RG Z x NUL (a stub of 40 bytes that is no record: its tags are malformed)
    out.append(("decoy: no tags, then the bytes RG Z x NUL", rec(b""), "none"))
    out.append(("decoy: the stub", TARGET + b"Zx\0" + bytes(35), "malformed"))
    # (d) l_seq says more than the record holds / is negative
    r = bytearray(rec(rg))
    struct.pack_into("<i", r, 20, 1000)
    out.append(("l_seq beyond the record", bytes(r), "malformed"))
    struct.pack_into("<i", r, 20, -1)
    out.append(("l_seq negative", bytes(r), "malformed"))
    out.append(("decoy: behind the damaged l_seq", rec(rg), found))
    return out


CASES = _cases()


def view(records):
    """(raw bytes, raw_start) of the records laid out back to back"""
    starts, at = [0], 0
    for r in records:
        at += len(r)
        starts.append(at)
    return b"".join(records), starts


def reference(raw, starts, tag=TARGET):
    """bam.find_tag of every record of a view; record k sees raw[:starts[k + 1]] - nothing behind its own end"""
    return [bam.find_tag(raw[:starts[k + 1]], starts[k], tag) for k in range(len(starts) - 1)]


def check_case(raw, start, end, got, want):
    """does got = (val_off, val_len, val_type) say what the construction of the case says"""
    off, ln, t = got
    if want == "none":
        return got == (-1, 0, 0)
    if want == "malformed":
        return got == (-2, 0, 0)
    _, value, letter = want
    return start <= off and off + ln <= end and raw[off:off + ln] == value and t == ord(letter) and ln == len(value)


def random_records(seed, n, damaged_every=3):
    """n records with random tag lists (RG at a random place or absent), every damaged_every-th one damaged: its tag bytes cut at a
    random place, or one of their bytes replaced"""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        tags = []
        for _ in range(rnd.randrange(0, 6)):
            name = bytes(rnd.choice(b"ABCDEFXYZ") for _ in range(2))
            kind = rnd.randrange(4)
            if kind == 0:
                t = rnd.choice("cCsSiI")
                lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-2 ** 15, 2 ** 15 - 1), "S": (0, 2 ** 16 - 1), "i": (-2 ** 31, 2 ** 31 - 1),
                          "I": (0, 2 ** 32 - 1)}[t]
                tags.append(scalar(name, t, rnd.randint(lo, hi)))
            elif kind == 1:
                tags.append(Z(name, bytes(rnd.randrange(33, 127) for _ in range(rnd.choice((0, 1, 5, 15, 16, 17, 40, 130))))))
            elif kind == 2:
                sub = rnd.choice("CSI")
                tags.append(B(name, sub, [rnd.randrange(0, 200) for _ in range(rnd.randrange(0, 40))]))
            else:
                tags.append(scalar(name, "A", bytes([rnd.randrange(33, 127)])))
        if rnd.random() < 0.7:
            tags.insert(rnd.randrange(len(tags) + 1), Z(TARGET, rnd.choice((b"a", b"ab", b"grp1", b"", b"x" * 30))))
        tags = b"".join(tags)
        if k % damaged_every == 0 and tags:
            if rnd.random() < 0.5:
                tags = tags[:rnd.randrange(len(tags))]
            else:
                at = rnd.randrange(len(tags))
                tags = tags[:at] + bytes([rnd.choice((0, 66, 90, 255, 105))]) + tags[at + 1:]
        seq = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 40)))
        out.append(rec(tags, name=b"read%d" % k, seq=seq))
    return out
