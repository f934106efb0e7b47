"""Windows of raw BAM record bytes for the tests of rd_bam_index (csrc/rd_bam_index.hpp) below the reader, and what a call on such a
window must produce - expect(), built from the rule's walk bam.records(window, start=0) alone. No GPU here: tests/test_bam_windows_host.py
proves, with the rule only, that the windows are what tests/test_gpu_bam_index.py assumes (where records start, where they do not, how
many segments of S = bam.SEGMENT bytes a window has), and that check(), the comparator of the GPU tests, rejects every single-entry
perturbation. The real bases of a window stay far below 50,000 (bam.records loops over bases in Python); the bulk is tag filler."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ribodetector_amd import _native as N  # noqa: E402
from ribodetector_amd import bam  # noqa: E402
import test_gpu_bam as G  # noqa: E402      (_read_of, _damaged, FAULTS: no GPU is touched by importing it)

S = bam.SEGMENT
LEAD = 36 + 5 + 3              # a host record named b"host": fixed fields, name + NUL, tag name and type - its Z payload starts LEAD bytes in
UNPRINTABLE = bytes(range(1, 33)) + bytes(range(127, 256))
LONG_NAME = bytes(33 + i % 94 for i in range(254))           # l_read_name = 255: the NUL lies 290 bytes behind the record's start
LONG_SIZE = 36 + 255
REACH_D = (1, 4, 36, 290, 291)


# ---- builders -------------------------------------------------------------------------------------------------------------------------
def filler(size, name=b"f"):
    """a record (bytes) of exactly `size` bytes (>= 41 + len(name)): no bases, a Z tag that fills it - of any size, several MiB included"""
    fill = size - (36 + len(name) + 1) - 4
    assert fill >= 0, size
    return bam.encode_record(dict(name=name, seq=b"", qual=b"", tags=b"XZZ" + b"z" * fill + b"\0"))


def unprintable(read, rng):
    """the read with a name of the same length (at least one byte) drawn from bytes 1..32 and 127..255: bam_plausible rejects its start"""
    out = dict(read)
    out["name"] = bytes(rng.choice(np.frombuffer(UNPRINTABLE, np.uint8), size=max(len(read["name"]), 1)))
    return out


def far_fields(rec):
    """the record (bytes) with refID / pos / next_refID / next_pos = -2: well-formed for the walk, rejected by bam_plausible"""
    out = bytearray(bam.encode_record(rec))
    for at in (4, 8, 24, 28):
        struct.pack_into("<i", out, at, -2)
    return bytes(out)


def tiny(n, named):
    """n records (bytes each) without bases: 37 bytes and 6 bytes of text with an empty name, 38 and 7 with a one-byte name"""
    return [bam.encode_record(dict(name=bytes([33 + i % 94]) if named else b"", seq=b"", qual=b"")) for i in range(n)]


def long_name():
    """the record with l_read_name = 255 (LONG_SIZE bytes)"""
    return bam.encode_record(dict(name=LONG_NAME, seq=b"", qual=b""))


def decoy_at(offset, rejoin):
    """(start, host, decoy): a host record (bytes) that, placed at `start` = offset - LEAD, holds in its Z tag a well-formed unmapped
    record `decoy` starting exactly at `offset`. rejoin: the decoy's block_size ends at the host's end - its chain meets the true one"""
    decoy = bytearray(bam.encode_record(dict(name=b"decoy", seq="ACGTACGTAC", qual=bytes(range(10, 20)))))
    tail = b"t" * 300
    if rejoin:
        struct.pack_into("<i", decoy, 0, len(decoy) - 4 + len(tail) + 1)
    host = bam.encode_record(dict(name=b"host", seq=b"", qual=b"", tags=b"XDZ" + bytes(decoy) + tail + b"\0"))
    assert host[LEAD:LEAD + len(decoy)] == bytes(decoy)
    return offset - LEAD, host, bytes(decoy)


class Chain:
    """records one behind the other. `at`: the offset of the next one. to(t) fills up to offset t with fillers of 48..3000 bytes and, as
    every 50th record, a read of the next test_gpu_bam._read_of kind (0..11 in turn: tags, reverse strand, absent qualities, CIGARs, the
    skipped flags 0x100 / 0x800), so that a record starts exactly at t. encode: dict -> bytes, for windows whose every start is guess-proof"""

    def __init__(self, seed):
        self.rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
        self.recs, self.at, self.n, self.kind = [], 0, 0, 0
        self.targets, self.decoys, self.spans = [], [], []

    def add(self, rec, encode=None):
        raw = rec if isinstance(rec, (bytes, bytearray)) else (encode or bam.encode_record)(rec)
        self.recs.append(bytes(raw))
        self.at += len(raw)
        return self

    def read(self, n_bases=None, encode=None):
        n_bases = int(self.rng.integers(1, 200)) if n_bases is None else n_bases
        self.add(G._read_of(self.rng, n_bases, kind=self.kind % 12), encode)
        self.kind += 1
        return self

    def to(self, t, encode=None, target=True):
        gap = t - self.at
        assert gap == 0 or gap >= 48, (self.at, t)
        while t - self.at > 6000:
            self.n += 1
            if self.n % 50 == 0:
                self.read(encode=encode)
            else:
                size, name = int(self.rng.integers(48, 3001)), b"f%d" % (self.n % 1000)
                self.add(dict(name=name, seq=b"", qual=b"", tags=b"XZZ" + b"z" * (size - 41 - len(name)) + b"\0"), encode)
        if t > self.at:
            self.add(dict(name=b"f", seq=b"", qual=b"", tags=b"XZZ" + b"z" * (t - self.at - 42) + b"\0"), encode)
        assert self.at == t
        if target:
            self.targets.append(t)
        return self

    def decoy(self, offset, rejoin):
        start, host, _ = decoy_at(offset, rejoin)
        self.to(start).add(host)
        self.decoys.append((offset, rejoin))
        return self

    def span(self, start, size):
        """a record of `size` bytes that starts at `start`"""
        self.to(start).add(filler(size, name=b"span"))
        self.spans.append((start, size))
        return self

    def window(self, cut=None):
        data = b"".join(self.recs)
        return Window(data if cut is None else data[:cut], self.targets, self.decoys, self.spans)


def place(targets, seed=0):
    """fillers and reads arranged so that a record starts exactly at each target offset: the records (bytes each) of [0, targets[-1])"""
    c = Chain(seed)
    for t in sorted(targets):
        c.to(t)
    return c.recs


class Window:
    """the bytes of one window and what its builder intends: offsets where records start, (offset, rejoin) of decoys, (start, size) of
    spanning records"""

    def __init__(self, data, targets=(), decoys=(), spans=()):
        self.data = data
        self.targets = [t for t in targets if t <= len(data)]
        self.decoys, self.spans = list(decoys), list(spans)

    @property
    def nseg(self):
        return len(self.data) // S + (len(self.data) % S != 0)


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def expect(window, final):
    """what rd_bam_index must produce on `window` (offsets counted from the window's begin), from the rule's serial walk alone"""
    recs, status, bad = [], 0, -1
    try:
        for r in bam.records(window, start=0):
            recs.append(r)
    except ValueError as e:
        if str(e) == bam.TRUNCATED:
            status = N.BAM_TRUNCATED if final else 0          # (a window that ends inside a record is no fault while more bytes may follow)
        else:
            assert str(e) == bam.MALFORMED % len(recs)
            status, bad = N.BAM_RECORD, len(recs)
    kept = [r for r in recs if not r.skipped]
    texts = [r.fastq() for r in kept]
    rec_tab = np.zeros(len(kept) + 1, np.int64)
    rec_tab[1:] = np.cumsum([len(t) for t in texts], dtype=np.int64)
    return dict(status=status, n_records=len(kept), n_lines=len(recs), consumed=recs[-1].offset + recs[-1].size if recs else 0, bad_record=bad,
                norm=b"".join(texts), rec_tab=rec_tab, hdr_tab=np.array([len(r.name) + 1 for r in kept], np.int32), offsets=[r.offset for r in recs])


FIELDS = ("status", "n_records", "n_lines", "consumed", "bad_record")


def check(got, want, tag=""):
    """the comparator of the GPU tests: every field of expect() (got: the same keys, read back from the device)"""
    for k in FIELDS:
        assert int(got[k]) == int(want[k]), "%s %s: %d, expected %d" % (tag, k, int(got[k]), int(want[k]))
    g, w = got["norm"], want["norm"]
    if g != w:
        first = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("%s norm: %d bytes, expected %d; first difference at byte %d" % (tag, len(g), len(w), first))
    for k in ("rec_tab", "hdr_tab"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), "%s %s differs%s" % (tag, k, "" if a.shape != b.shape else " first at entry %d" % int(np.flatnonzero(a != b)[0]))


# ---- the windows of the cases ---------------------------------------------------------------------------------------------------------
ROUND_EDGES = [64 * S - 1, 64 * S, 64 * S + 1, 128 * S - 1, 128 * S, 128 * S + 1, 64 * S + S // 2 + 7, 128 * S + 12345]


def round_edge(length):
    """a clean chain of exactly `length` bytes; where there is room, a record ends (and the next starts) exactly at 64 S and 128 S"""
    c = Chain(100 + length % 997)
    for t in (64 * S, 128 * S):
        if 48 <= length - t or length == t:
            c.to(t)
    return c.to(length).window()


DECOY_J = (1, 63, 64, 65, 127, 128)
TWO_DECOYS = ((63, False, 65, True), (1, True, 127, False))       # serial then serial; serial, then serial again behind it


def decoys(js, rejoins, n=130):
    """decoys at j S for the j of `js`, alone in a window of n segments"""
    c = Chain(200 + 7 * js[0] + rejoins[0])
    for j, rj in zip(js, rejoins):
        c.decoy(j * S, rj)
    return c.to(n * S - 77).window()


SPANS = {"62_to_66": (62 * S + 1000, 4 * S - 500, 70), "60_to_130": (60 * S + 31000, 70 * S - 30000, 133), "0_for_70": (2 * 1024 + 48, 70 * S, 73)}


def spanning(tag):
    start, size, n = SPANS[tag]
    c = Chain(300 + len(tag))
    for _ in range(3):
        c.read()
    c.span(start, size)
    for _ in range(3):
        c.read()
    return c.to(n * S - 501).window()


def guess_proof(how):
    """70 segments whose every record start bam_plausible rejects: unprintable names, or far fields"""
    c = Chain(400 + len(how))
    rng = np.random.default_rng(401)
    enc = (lambda r: bam.encode_record(unprintable(r, rng))) if how == "unprintable" else far_fields
    return c.to(70 * S - 333, encode=enc).window()


def dense(behind):
    """40,000 records of 37 bytes (segment lists filled to their last entry), from offset 0 or behind 64 segments of fillers"""
    c = Chain(500)
    if behind:
        c.to(64 * S + 11)
    for r in tiny(40000, named=False):
        c.add(r)
    return c.window()


def reach(h, d, how):
    """the l_read_name = 255 record at h - d. how: "mid" (reads behind it), "last" (the window's last record), "cut" (the window ends
    inside its name)"""
    c = Chain(600 + d)
    c.to(h - d).add(long_name())
    if how == "mid":
        for _ in range(4):
            c.read()
        c.to(c.at + 700)
    return c.window(cut=h - d + 36 + 100 if how == "cut" else None)


def ends_chain():
    """the 66-segment chain of the Ends cases and (offset, size) of a record of segment 65"""
    c = Chain(700)
    w = c.to(66 * S - 4000).window()
    at = 0
    for r in c.recs:
        if at >= 65 * S + 3000:
            return w, at, len(r)
        at += len(r)
    raise AssertionError("no record in segment 65")


def damaged(what, decoy=False):
    """good records for 64 segments and more (some with flag 0x100 / 0x800), then the fault of test_gpu_bam._damaged - behind a decoy at
    64 S when asked, the fault in the segment right after it - and 20 good records unless the fault is a cut"""
    c = Chain(800 + G.FAULTS.index(what))
    if decoy:
        c.decoy(64 * S, False)
    c.to(65 * S + 1000 + 100 * G.FAULTS.index(what))
    rng = np.random.default_rng(801)
    c.add(G._damaged(what, bam.encode_record(G._read_of(rng, 80, name=b"damaged", kind=5))))
    if not what.startswith("cut"):
        for _ in range(20):
            c.read()
    return c.window()


def ordinary():
    """a 66-segment chain whose text is NOT a multiple of 16 bytes long (the byte tail of the emit pass at norm_cap = its length)"""
    c = Chain(900).to(66 * S - 1234)
    T = len(expect(c.window().data, 1)["norm"])
    return c.add(dict(name=b"x" * ((5 - T - 6) % 16), seq=b"", qual=b"")).window()


def sweep(seed):
    """(window, final): 66-70 segments that mix everything above at random, with record starts landing within 4 bytes of segment
    boundaries, a random final and a random end (a record's end, inside a record, inside a block_size, a fault)"""
    rng = np.random.default_rng(10_000 + seed)
    c = Chain(rng)
    total = int(rng.integers(65 * S + 8000, 70 * S - 8000))
    enc_u, enc_f = (lambda r: bam.encode_record(unprintable(r, rng))), far_fields
    while c.at < total - 5 * S:
        what, k = int(rng.integers(0, 9)), c.at // S + 2
        if what == 0:
            c.to(c.at + int(rng.integers(S // 2, 3 * S)))
        elif what == 1:
            c.to(k * S + int(rng.integers(-4, 5))).read()
        elif what == 2:
            c.decoy(k * S, bool(rng.integers(0, 2)))
        elif what == 3:
            c.span(c.at, int(rng.integers(S, 3 * S)))
        elif what in (4, 5):
            c.to(c.at + int(rng.integers(S, 2 * S)), encode=enc_u if what == 4 else enc_f)
        elif what == 6:
            for r in tiny(int(rng.integers(100, 3000)), named=bool(rng.integers(0, 2))):
                c.add(r)
        elif what == 7:
            c.to(k * S - int(rng.choice(REACH_D))).add(long_name())
        else:
            for _ in range(5):
                c.read()
    c.to(total)
    end, cut = int(rng.integers(0, 5)), None
    size = len(c.recs[-1])
    if end == 1:
        cut = c.at - size + int(rng.integers(4, size))
    elif end == 2:
        cut = c.at - size + int(rng.integers(1, 4))
    elif end == 3:
        cut = c.at - size
    elif end == 4:
        what = G.FAULTS[int(rng.integers(0, len(G.FAULTS)))]
        c.add(G._damaged(what, bam.encode_record(G._read_of(rng, 80, name=b"damaged", kind=5))))
        if not what.startswith("cut"):
            for _ in range(5):
                c.read()
    return c.window(cut), int(rng.integers(0, 2))
