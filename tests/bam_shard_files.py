"""Inputs of the --bam_shard tests (tests/test_bam_shard_host.py, tests/test_gpu_bam_shard.py): record mixes, the decoys that the rule
of bam.find_record_start does and does not accept, and the reference answers, from bam.records alone. No GPU here."""
import struct

import numpy as np

from ribodetector_amd import bam

LONG_NAME = bytes(33 + i % 94 for i in range(254))           # l_read_name = 255


def seq_of(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) if n else b""


def read_of(rng, n_bases, name, **kw):
    return dict(name=name, seq=seq_of(rng, n_bases), qual=bytes(rng.integers(0, 42, size=n_bases, dtype=np.uint8)), **kw)


def mixed_reads(seed, n=1200, big=2):
    """n reads that mix the shapes the rule must hold on: no bases, 37-byte records (no name, no bases), 100 bp, reverse strand, the
    skipped flags 0x100 / 0x800, tags, 255-byte names, mapped records with CIGARs - and `big` records of 70,000 bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = i % 12
        name = b"r%d" % i
        if k == 0:
            out.append(read_of(rng, 0, name))
        elif k == 1:
            out.append(dict(name=b"", seq=b"", qual=b""))
        elif k == 2:
            out.append(read_of(rng, 100, name, flag=0x10))
        elif k == 3:
            out.append(read_of(rng, 100, name, flag=0x100))
        elif k == 4:
            out.append(read_of(rng, 100, name, flag=0x800 | 0x10))
        elif k == 5:
            out.append(read_of(rng, 100, name, tags=b"RGZgrp%d\0" % (i % 5) + b"NMC\x03" + b"XBBS" + struct.pack("<I", 3) + b"\1\0\2\0\3\0"))
        elif k == 6:
            out.append(read_of(rng, 61, LONG_NAME))
        elif k == 7:
            out.append(read_of(rng, 100, name, flag=0, ref_id=0, pos=1000 + i, mapq=30, cigar=[(60, "M"), (2, "I"), (38, "M")]))
        elif k == 8:
            out.append(dict(name=name, seq=seq_of(rng, 75), qual=None))
        else:
            out.append(read_of(rng, int(rng.integers(1, 151)), name))
    for j in range(big):
        out.insert((j + 1) * n // (big + 1), read_of(rng, 70000, b"big%d" % j))
    return out


def small_reads(seed, n, lo=60, hi=150, groups=0, skipped_every=0, prefix=b"s"):
    """n reads of lo..hi bases; groups: RG:Z tags over that many ids; skipped_every: a 0x900 record in front of every k-th read"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if skipped_every and i % skipped_every == 0:
            out.append(read_of(rng, 50, b"%ssup%d" % (prefix, i), flag=0x800))
        kw = dict(tags=b"RGZg%02d\0" % (i % groups)) if groups else {}
        out.append(read_of(rng, int(rng.integers(lo, hi + 1)), b"%s%d" % (prefix, i), **kw))
    return out


DECOY = bam.encode_record(dict(name=b"decoy", seq="ACGTACGTAC", qual=bytes(range(10, 20))))
NOISE = b"\xff" * 64


def decoy_host(k, noise=True):
    """(record bytes, offset of the payload in it): a record whose B:C tag holds k byte-identical well-formed records and then (noise)
    64 bytes of 0xff, so that the chain behind the k-th lands on no record - not on the start of the record behind the host either"""
    payload = DECOY * k + (NOISE if noise else b"")
    rec = bam.encode_record(dict(name=b"host", seq=b"", qual=b"", tags=b"XBBC" + struct.pack("<I", len(payload)) + payload))
    at = 36 + 5 + 3 + 1 + 4
    assert rec[at:at + len(payload)] == payload
    return rec, at


def with_host(k, noise=True):
    """(bytes of 5 reads, the host of k decoys, 12 reads; offset of the host, of its payload, of the record behind it)"""
    rng = np.random.default_rng(13)
    head = [bam.encode_record(r) for r in small_reads(14, 5)]
    host, at = decoy_host(k, noise)
    tail = [bam.encode_record(read_of(rng, 80, b"t%d" % i)) for i in range(12)]
    h0 = sum(len(r) for r in head)
    return b"".join(head) + host + b"".join(tail), h0, h0 + at, h0 + len(host)


def skipped_filler(size, name=b"fill"):
    """a supplementary record (not delivered) of exactly `size` bytes (>= 45 + len(name)): no bases, a Z tag that fills it"""
    fill = size - (36 + len(name) + 1) - 4
    assert fill >= 0, size
    return bam.encode_record(dict(name=name, seq=b"", qual=b"", flag=0x800, tags=b"XZZ" + b"z" * fill + b"\0"))


def starts_of(data, start=None):
    """(offsets of every record of the walk - the skipped ones included -, which of them are delivered), by bam.records"""
    recs = list(bam.records(data, start))
    return [r.offset for r in recs], [not r.skipped for r in recs]


def accepted(data, lo, first=1 << 13):
    """what a caller of bam.find_record_start accepts for `lo`: windows [.., lo + first), fourfold while undecided; len(data) = none"""
    n = first
    while True:
        end = min(len(data), lo + n)
        found, und = bam.find_record_start(data[:end], lo, end, end == len(data))
        if found >= 0 and (und < 0 or und > found):
            return found
        if end == len(data):
            assert und < 0
            return len(data)
        n *= 4
