"""BAM input on the GPU. The oracle everywhere is ribodetector_amd/bam.py (fastq_text: the plain serial walk) plus the existing FASTQ
path: the chunks of a BAM file must equal, byte for byte and table for table, the chunks of the plain FASTQ file of bam.fastq_text of
the same bytes, and a CLI run on a BAM file the run on that FASTQ file. S = bam.SEGMENT: rd_bam_index frames a batch in segments of S
bytes counted from the batch's first record - in a file of one batch, from the first record of the file."""
import gzip
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_interleaved_host as H  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = bam.SEGMENT
NAME_BYTES = bytes(range(33, 127))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _read_of(rng, n_bases, name=None, kind=None):
    """one read with everything the format allows that the text must ignore or obey: tags, reverse strand, absent qualities, a mapped
    record with a CIGAR, secondary / supplementary flags"""
    if name is None:
        name = bytes(rng.choice(np.frombuffer(NAME_BYTES, np.uint8), size=int(rng.integers(0, 40))))
    seq = bytes(rng.choice(np.frombuffer(bam.CODES, np.uint8), size=n_bases, p=[0.01, 0.22, 0.22, 0.01, 0.22, 0.01, 0.01, 0.01, 0.22, 0.01, 0.01, 0.01, 0.01, 0.01, 0.01, 0.01]))
    read = dict(name=name, seq=seq, qual=bytes(rng.integers(0, 100, n_bases, dtype=np.uint8)))
    kind = int(rng.integers(0, 12)) if kind is None else kind
    if kind == 0:
        read["qual"] = None
    elif kind == 1:
        read["flag"] = 0x10
    elif kind == 2:
        read.update(flag=0x10 | 0x1 | 0x80, ref_id=0, pos=int(rng.integers(0, 1 << 20)), mapq=60, cigar=[(max(n_bases - 3, 0), "M"), (min(n_bases, 3), "S")],
                    next_ref_id=0, next_pos=7, tlen=-300)
    elif kind == 3:
        read.update(flag=0x100, ref_id=0, pos=5, cigar=[(n_bases, "M")])
    elif kind == 4:
        read.update(flag=0x800 | 0x10, ref_id=1, pos=9, cigar=[(n_bases, "M"), (5, "H")])
    if kind % 3 == 0:
        read["tags"] = b"RGZgrp1\0" + b"NMC\x03" + b"XBBC" + struct.pack("<i", 16) + bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    return read


def _sized(size, name=b"f"):
    """a record of exactly `size` bytes (>= 48): no bases, a Z tag that fills it"""
    fill = size - (36 + len(name) + 1) - 4
    assert fill >= 0
    return dict(name=name, seq=b"", qual=b"", tags=b"XZZ" + b"z" * fill + b"\0")


def _files(tmp_path, tag, reads, **kw):
    """(path of the BAM file, path of the FASTQ file of its rule text, the inflated bytes)"""
    b, f = str(tmp_path / (tag + ".bam")), str(tmp_path / (tag + ".fq"))
    data = bam.write_bam(b, reads, **kw)
    open(f, "wb").write(bam.fastq_text(data))
    return b, f, data


def _chunks(path, chunk, stats=None, errors=None):
    from ribodetector_amd.data_loader import device_reader as dr
    out = []
    try:
        for c in dr.get_seq_chunks_device(path, chunk_size=chunk, first_chunk=chunk, device=DEV, stats=stats):
            text, rs, so, sl = c.to_host()
            assert len(rs) == c.n + 1 and len(so) == len(sl) == c.n and rs[0] == 0 and rs[-1] == len(text)
            out.append((text.tobytes(), rs, so, sl))
    except ValueError as e:
        if errors is None:
            raise
        errors.append(str(e))
    return out


def _same(tmp_path, tag, reads, chunk=500, **kw):
    """the BAM file's chunks = the chunks of the FASTQ file of the rule's text; returns the indexer's counters"""
    b, f, data = _files(tmp_path, tag, reads, **kw)
    st = {}
    got, want = _chunks(b, chunk, stats=st), _chunks(f, chunk)
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "%s chunk %d: text differs" % (tag, k)
        for a, c, what in ((g[1], w[1], "rec_start"), (g[2], w[2], "seq_off"), (g[3], w[3], "seq_len")):
            assert a.dtype == c.dtype and np.array_equal(a, c), "%s chunk %d: %s differs" % (tag, k, what)
    recs = list(bam.records(data))
    ix = st["indexer"]
    assert ix["bam_records"] == len(recs) and ix["bam_skipped"] == sum(r.skipped for r in recs)
    assert b"".join(g[0] for g in got) == bam.fastq_text(data)
    return ix


@pytest.fixture
def small_batches(monkeypatch):
    """(first, members): the compressed bytes of the first batch and the members per batch; light pinned buffers"""
    from ribodetector_amd.data_loader import device_reader as dr

    def set_sizes(first, members):
        monkeypatch.setattr(dr.DeviceFeeder, "FIRST", first)
        monkeypatch.setattr(dr.DeviceFeeder, "BATCH", 1 << 20)
        monkeypatch.setattr(dr.DeviceFeeder, "MAX_MEMBERS", members)
    return set_sizes


# ---- the indexer against the rule -----------------------------------------------------------------------------------------------------
def test_a_seeded_records_of_every_kind(tmp_path):
    rng = np.random.default_rng(20)
    reads = [_read_of(rng, int(rng.integers(1, 301))) for _ in range(3000)]
    ix = _same(tmp_path, "a", reads, refs=[(b"chr1", 1 << 24), (b"chr2", 1000)], text=b"@HD\tVN:1.6\tSO:unsorted\n")
    assert ix["bam_skipped"] > 100 and ix["batches"] >= 2


def test_b_record_starts_around_every_segment_boundary(tmp_path):
    """a record start at each of k S - 4 ... k S + 4: block_size and the fixed fields lie across a segment boundary"""
    rng = np.random.default_rng(21)
    reads, at, targets = [], 0, [k * S + d for k, d in zip(range(1, 10), range(-4, 5))]
    for t in targets:
        while t - at > 4000:
            reads.append(_read_of(rng, int(rng.integers(200, 900))))
            at += len(bam.encode_record(reads[-1]))
        reads.append(_sized(t - at))
        at = t
        reads.append(_read_of(rng, 150, kind=0 if t % 2 else 1))      # the record that starts at the target
        at += len(bam.encode_record(reads[-1]))
    data = bam.payload(reads)
    offs = {r.offset - bam.header_len(data) for r in bam.records(data)}
    assert all(t in offs for t in targets)
    _same(tmp_path, "b", reads)


def test_c_records_longer_than_segments(tmp_path):
    """a record of 5 S bytes between short ones (segments without any entry), and 2 S bases without qualities (a long run of 0xFF)"""
    rng = np.random.default_rng(22)
    short = lambda n: [_read_of(rng, int(rng.integers(30, 200))) for _ in range(n)]      # noqa: E731
    n5 = (5 * S - 50) * 2 // 3
    reads = short(40) + [_read_of(rng, n5, name=b"five_segments", kind=1)] + short(40) + [_read_of(rng, 2 * S, name=b"no_quals", kind=0)] + short(40)
    assert 5 * S - 8 <= len(bam.encode_record(reads[40])) <= 5 * S + 8
    _same(tmp_path, "c", reads, chunk=50)


def _decoy_reads(rng, rejoin):
    """a record whose Z tag holds, byte for byte, a well-formed unmapped record, placed so that it starts exactly at a segment boundary:
    the speculative framing of that segment starts at the decoy, the in-order pass has to walk the segment again. rejoin: the decoy's
    block_size ends at the end of the record that holds it - its chain meets the true one there"""
    reads, at = [], 0
    while 2 * S - at > 6000:
        reads.append(_read_of(rng, int(rng.integers(200, 900))))
        at += len(bam.encode_record(reads[-1]))
    host_name, lead = b"host", 36 + 5 + 3                   # fixed fields, name + NUL, tag name and type: the payload starts `lead` bytes in
    reads.append(_sized(2 * S - lead - at - 600))
    at = 2 * S - lead - 600
    reads.append(_sized(600, name=b"g"))                     # (a record start 600 bytes in front: the host starts at 2 S - lead)
    decoy = bytearray(bam.encode_record(dict(name=b"decoy", seq="ACGTACGTAC", qual=bytes(range(10, 20)))))
    tail = b"t" * 300
    if rejoin:                                               # the decoy claims everything up to the host's end: the tag's tail and its NUL
        struct.pack_into("<i", decoy, 0, len(decoy) - 4 + len(tail) + 1)
    reads.append(dict(name=host_name, seq=b"", qual=b"", tags=b"XDZ" + bytes(decoy) + tail + b"\0"))
    reads += [_read_of(rng, int(rng.integers(50, 300))) for _ in range(200)]
    data = bam.payload(reads)
    hdr = bam.header_len(data)
    assert data[hdr + 2 * S:hdr + 2 * S + len(decoy)] == bytes(decoy) and 2 * S not in {r.offset - hdr for r in bam.records(data)}
    assert [r.name for r in bam.records(bytes(decoy) + (tail + b"\0" if rejoin else b""), start=0)] == [b"decoy"]
    return reads


@pytest.mark.parametrize("rejoin", [False, True])
def test_d_a_decoy_record_in_a_tag_at_a_segment_boundary(tmp_path, rejoin):
    ix = _same(tmp_path, "d%d" % rejoin, _decoy_reads(np.random.default_rng(23), rejoin))
    assert ix["bam_rewalked_segments"] >= 1


def test_e_batch_boundaries_inside_records(tmp_path, small_batches):
    """one member per batch: batches end inside a record, inside the 4 bytes of block_size and exactly on a record start; one record is
    larger than a whole batch (its carry grows over many batches)"""
    rng = np.random.default_rng(24)
    reads = [_read_of(rng, int(rng.integers(20, 120))) for _ in range(60)]
    reads.insert(30, _read_of(rng, 3000, name=b"longer_than_a_batch", kind=1))
    data = bam.payload(reads)
    offs = [r.offset for r in bam.records(data)]
    cuts = [offs[3], offs[5] + 2, offs[8] + 50, offs[9], offs[12] + 1, offs[12] + 3, offs[12] + 4, offs[12] + 36]
    sizes = [b - a for a, b in zip([0] + cuts, cuts)] + [211]
    assert all(s > 0 for s in sizes)
    small_batches(1 << 12, 1)
    ix = _same(tmp_path, "e", reads, chunk=16, member_bytes=sizes)
    assert ix["batches"] > 20


def test_f_members_of_every_kind(tmp_path, small_batches):
    rng = np.random.default_rng(25)
    reads = [_read_of(rng, int(rng.integers(1, 301))) for _ in range(400)]
    text = b"".join(b"@SQ\tSN:contig%06d\tLN:%d\n" % (i, 1000 + i) for i in range(7400))       # > 200 KiB: the header spans members
    _same(tmp_path, "f_big", reads, member_bytes=0xff00, level=9)
    _same(tmp_path, "f_stored", reads, level=0, text=text)
    _same(tmp_path, "f_hdr", reads, text=text, refs=[(b"contig%06d" % i, 1000 + i) for i in range(50)], member_bytes=[0xff00, 0xff00, 5000, 0, 1, 1, 1, 0, 777])
    small_batches(1 << 12, 3)            # (the header spans batches too)
    _same(tmp_path, "f_hdr_batches", reads[:100], text=text, member_bytes=[3000])
    # one-byte members through the first records, an empty member mid-file
    small_batches(1 << 16, 4096)
    data = bam.payload(reads[:40])
    _same(tmp_path, "f_tiny", reads[:40], member_bytes=[1] * 300 + [0, 0, 913])
    # a Tail: a plain gzip member (no size field) appended - the rest of the file goes through zlib on the host, into the same indexer
    b, f, _ = _files(tmp_path, "f_tail", reads[:40])
    more = b"".join(bam.encode_record(r) for r in reads[40:90])
    raw = open(b, "rb").read()
    assert raw.endswith(bam.EOF_MEMBER)
    open(b, "wb").write(raw[:-28] + gzip.compress(more[:1000], 6) + gzip.compress(more[1000:], 1))
    open(f, "wb").write(bam.fastq_text(data + more))
    assert [c[0] for c in _chunks(b, 32)] == [c[0] for c in _chunks(f, 32)]
    # ... and a file that is no BGZF at all (one gzip stream): the tail route from its first byte, the header dropped there
    open(b, "wb").write(gzip.compress(data + more, 6))
    assert [c[0] for c in _chunks(b, 32)] == [c[0] for c in _chunks(f, 32)]


def test_g_empty_and_headerless_damage(tmp_path):
    b = str(tmp_path / "empty.bam")
    bam.write_bam(b, [], refs=[(b"chr1", 5)], text=b"@HD\tVN:1.6\n")
    assert _chunks(b, 100) == []
    bam.write_bam(b, [], eof=False)                                # (a missing end-of-file member is tolerated)
    assert _chunks(b, 100) == []
    rng = np.random.default_rng(26)
    reads = [_read_of(rng, 50) for _ in range(10)]
    bam.write_bam(b, reads, eof=False)
    assert b"".join(c[0] for c in _chunks(b, 100)) == bam.fastq_text(bam.payload(reads))
    for raw, msg in ((bam.bgzf_member(b"BAM\2" + bytes(100)), "not a BAM file"), (bam.bgzf_member(bam.encode_header([(b"chr1", 5)])[:-2]), "truncated BAM header")):
        open(b, "wb").write(raw + bam.EOF_MEMBER)
        err = []
        assert _chunks(b, 100, errors=err) == [] and msg in err[0]


# ---- faults are reported, not followed ------------------------------------------------------------------------------------------------
def _damaged(what, rec):
    """the bytes that follow the good records"""
    if what.startswith("block="):
        return struct.pack("<i", int(what[6:], 0)) + rec[4:]
    if what == "l_read_name=0":
        return rec[:12] + b"\0" + rec[13:]
    if what == "no_nul":
        return rec[:36] + rec[36:].replace(b"\0", b"x", 1)
    if what == "l_seq":
        return rec[:20] + struct.pack("<I", 100000) + rec[24:]
    if what == "cut_in_record":
        return rec[:-7]
    assert what == "cut_in_block_size"
    return rec[:2]


FAULTS = ["block=0", "block=31", "block=-1", "block=0x7fffffff", "l_read_name=0", "no_nul", "l_seq", "cut_in_record", "cut_in_block_size"]


@pytest.mark.parametrize("what", FAULTS)
def test_faults_are_reported_not_followed(tmp_path, what):
    """the chunks in front of the damage, then the ValueError of the rule's own walk; the process stays healthy"""
    rng = np.random.default_rng(27)
    n, chunk = 300, 64
    good = [_read_of(rng, int(rng.integers(20, 150)), kind=int(rng.integers(0, 3))) for _ in range(n)]       # (none skipped)
    rec = bam.encode_record(_read_of(rng, 80, name=b"damaged", kind=5))
    after = b"" if what.startswith("cut") else b"".join(bam.encode_record(r) for r in good[:20])
    data = bam.payload(good) + _damaged(what, rec) + after
    with pytest.raises(ValueError) as e:
        list(bam.records(data))
    want = str(e.value)
    assert want == ("truncated BAM record at end of file" if what.startswith("cut") or what == "block=0x7fffffff" else "malformed BAM record %d" % n)
    b = str(tmp_path / "damaged.bam")
    with open(b, "wb") as fh:
        for p in range(0, len(data), 0xff00):
            fh.write(bam.bgzf_member(data[p:p + 0xff00]))
        fh.write(bam.EOF_MEMBER)
    err = []
    got = _chunks(b, chunk, errors=err)
    assert err == [want]
    text = bam.fastq_text(bam.payload(good))
    lines = text.split(b"\n")
    head = b"\n".join(lines[:4 * (n // chunk) * chunk]) + b"\n"       # whole chunks in front of the damage, as the FASTQ readers deliver them
    assert len(got) == n // chunk and b"".join(g[0] for g in got) == head
    _same(tmp_path, "healthy", good[:100], chunk=chunk)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
SMALL = ["--chunk_size", "1", "-m", "3"]


def _read(path):
    if not os.path.exists(path):
        return None
    with (gzip.open if path.endswith("gz") else open)(path, "rb") as fh:
        return fh.read()


def _run(args, env=None):
    from ribodetector_amd import detect
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return detect.main(args)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bam_reads(arena, off, mate=None, rng=None):
    """synthetic reads as BAM records: some on the reverse strand (stored reverse-complemented, so that the text is the read again)"""
    raw, out = arena.tobytes(), []
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    for i in range(len(off) - 1):
        s = raw[off[i]:off[i + 1]]
        name = b"syn.%d" % i + (b"/%d" % mate if mate else b"")
        q = bytes(int(x) for x in ((np.arange(len(s)) * 7 + i) % 41))
        if rng is not None and rng.integers(0, 4) == 0:
            out.append(dict(name=name, seq=s.translate(comp)[::-1], qual=q[::-1], flag=0x10 | 0x4))
        else:
            out.append(dict(name=name, seq=s, qual=q))
    return out


def _pair_of_runs(tmp_path, tag, bam_inputs, fq_inputs, outs, extra=(), gz_out=False):
    """the same arguments over the BAM inputs and over the FASTQ inputs: every file the runs write must be the same bytes"""
    res = []
    for kind, inputs in (("bam", bam_inputs), ("fq", fq_inputs)):
        d = tmp_path / ("%s_%s" % (tag, kind))
        d.mkdir()
        ext = ".fq.gz" if gz_out else ".fq"
        o, r = [str(d / ("o%d%s" % (k, ext))) for k in range(outs)], [str(d / ("r%d%s" % (k, ext))) for k in range(outs)]
        rep, summ = str(d / "rep.tsv"), str(d / "summary.json")
        p = _run(["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "--read_report", rep, "--summary", summ] +
                 [str(d / a[5:]) if a.startswith("PATH:") else a for a in extra] + SMALL)
        doc = json.load(open(summ))
        assert doc.pop("inputs") == list(inputs)
        files = {os.path.basename(x): _read(x) for x in o + r + [rep] + [x + ".unclassified.gz" for x in o] + [str(d / "regions.bed")]}
        res.append((p, files, doc, (p.num_read, p.num_nonrrna, p.num_rrna, p.num_unknown)))
    (pb, fb, db, cb), (pf, ff, df, cf) = res
    assert cb == cf and db == df
    assert fb.keys() == ff.keys() and all(fb[k] == ff[k] for k in fb), [k for k in fb if fb[k] != ff[k]]
    assert all(v["path"] == "device" for v in pb.ingest.values())
    return pb, fb


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the 3,000 single-end reads of test_gpu_cli.test_cli_paired's first mate (their margins are known) and 1,000 synthetic pairs, as BAM files (write_bam) and as the FASTQ files of the rule's text"""
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("bamsets")
    rng = np.random.default_rng(30)
    out = {"dir": d}
    a, o, ln = synth.reads_numpy(3000, (60, 120), seed=41, rrna_frac=0.3)
    out["se"] = _files(d, "se", _bam_reads(a, o, rng=rng))[:2]
    out["se_arrays"] = (a, o, ln)
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(1000, (60, 120), seed=32, rrna_frac=0.3), synth.reads_numpy(1000, (60, 120), seed=33, rrna_frac=0.3)
    r1, r2 = _bam_reads(a1, o1, mate=1, rng=rng), _bam_reads(a2, o2, mate=2, rng=rng)
    out["r"] = (r1, r2)
    out["m1"], out["m2"] = _files(d, "m1", r1, text=b"@HD\tVN:1.6\n")[:2], _files(d, "m2", r2)[:2]
    out["il"] = _files(d, "il", H.interleave(r1, r2))[:2]
    return out


@pytest.mark.parametrize("gz_out", [False, True])
def test_cli_single_end(tmp_path, sets, gz_out):
    p, files = _pair_of_runs(tmp_path, "se", [sets["se"][0]], [sets["se"][1]], 1, gz_out=gz_out)
    assert p.num_read == 3000 and min(len(files["o0.fq" + (".gz" if gz_out else "")]), len(files["r0.fq" + (".gz" if gz_out else "")])) > 0
    assert p.ingest["se.bam"]["indexer"]["bam_records"] == 3000


def test_cli_single_end_stands_on_the_oracle(tmp_path, sets, oracle):
    """the labels of the BAM run against the oracle's, with the margin assertion of test_gpu_cli"""
    a, o, ln = sets["se_arrays"]
    g = oracle.forward_packed(a, o, ln, 100)
    assert np.abs(g[:, 1] - g[:, 0]).min() > 2e-4
    lab = oracle.argmax(g)
    lines = open(sets["se"][1], "rb").read().split(b"\n")
    recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]
    raw = a.tobytes()
    assert all(recs[i].split(b"\n")[1] == raw[o[i]:o[i + 1]] for i in range(0, 3000, 37))      # (reverse-strand records read as the read again)
    out, rr = str(tmp_path / "o.fq"), str(tmp_path / "r.fq")
    p = _run(["-l", "100", "-i", sets["se"][0], "-o", out, "-r", rr] + SMALL)
    assert p.num_read == 3000 and p.num_nonrrna == int((lab == 0).sum()) and p.num_rrna == int((lab == 1).sum())
    assert _read(out) == b"".join(recs[i] for i in np.flatnonzero(lab == 0)) and _read(rr) == b"".join(recs[i] for i in np.flatnonzero(lab == 1))


@pytest.mark.parametrize("ensure", ["rrna", "both"])
def test_cli_two_files(tmp_path, sets, ensure):
    p, files = _pair_of_runs(tmp_path, "pe_" + ensure, [sets["m1"][0], sets["m2"][0]], [sets["m1"][1], sets["m2"][1]], 2, extra=["-e", ensure])
    assert p.is_paired and p.num_read == 1000 and (files["o0.fq.unclassified.gz"] is not None) == (ensure == "both")


@pytest.mark.parametrize("outs", [1, 2])
def test_cli_interleaved(tmp_path, sets, outs):
    p, files = _pair_of_runs(tmp_path, "il%d" % outs, [sets["il"][0]], [sets["il"][1]], outs, extra=["--interleaved", "-e", "both"], gz_out=outs == 2)
    assert p.is_paired and p.num_read == 1000


def test_cli_interleaved_deleted_mate(tmp_path, sets):
    r1, r2 = sets["r"]
    recs = H.interleave(r1, r2)
    del recs[2 * 700]                                     # pair 700 loses its mate 1: records 1401 and 1402 (1-based) are not mates
    recs.append(dict(name=b"syn.tail", seq="ACGT", qual=b"\x28" * 4))
    b = str(tmp_path / "del.ubam")
    bam.write_bam(b, recs)
    o = str(tmp_path / "o.fq")
    with pytest.raises(RuntimeError) as e:
        _run(["-l", "100", "-i", b, "--interleaved", "-o", o] + SMALL)
    msg = str(e.value)
    assert "records 1401 and 1402" in msg and "'syn.700/2'" in msg and "'syn.701/1'" in msg
    assert len(_read(o)) > 0                             # (the first chunk's pairs were written)


def test_cli_windows_and_regions_on_long_records(tmp_path):
    from ribodetector_amd import synth
    rng = np.random.default_rng(34)
    a, o, _ = synth.reads_numpy(300, (250, 5000), seed=35, rrna_frac=0.4)
    b, f, _ = _files(tmp_path, "long", _bam_reads(a, o, rng=rng))
    p, files = _pair_of_runs(tmp_path, "win", [b], [f], 1, extra=["--windows", "--regions", "PATH:regions.bed"])
    assert p.num_read == 300 and files["regions.bed"] is not None and len(files["regions.bed"]) > 0


# ---- the reader over what tests/test_gpu_bam_index.py tests below it (windows of tests/bam_windows.py) -------------------------------------
@pytest.mark.parametrize("named", [False, True])
def test_h_records_without_bases_overflow_the_first_tables(tmp_path, named):
    """20,000 records of 37 (38) bytes: more than the window / 96 + 4096 entries of the batch's first tables - rd_bam_index refuses the
    batch (RD_FQ_LINES), BamIndexer frames it again with full-size tables"""
    import bam_windows as W
    ix = _same(tmp_path, "h%d" % named, W.tiny(20000, named))
    assert ix["reframed"] >= 1 and ix["bam_records"] == 20000


def test_i_two_decoys_in_different_rounds_of_one_batch(tmp_path):
    """about 140 segments in one batch: the stitch takes three rounds of 64 segments, a decoy in the first and one in the second"""
    import bam_windows as W
    c = W.Chain(29).decoy(40 * S, False).decoy(100 * S, True).to(140 * S - 999)
    ix = _same(tmp_path, "i", c.recs)
    assert ix["bam_rewalked_segments"] >= 2 and ix["batches"] == 2        # (the batch of the data and the empty one that ends every stream)
