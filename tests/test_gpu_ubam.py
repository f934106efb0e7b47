"""--ubam_output on the GPU. Kernel tests: rd_bam_encode (csrc/rd_bam_encode.hpp) on chunks built here - text and the three tables
a device chunk carries - compared with bam.from_fastq byte for byte: the raw bytes, raw_start and info, into a buffer with a guard
pattern behind its capacity. CLI tests: the same command without the flag (FASTQ / FASTA outputs) and with it; every .bam inflated
member by member with zlib and held against the header plus bam.from_fastq of the corresponding text output.

Launch shapes the sweep is sized by: the length and offsets passes take 2,048 records per workgroup (70,000 records: 35 workgroups);
the write pass owns 16 KiB of output per workgroup and trip and has at most 1,024 workgroups - the sweep's 70,000 records of 0..300
bases are about 1,200 tiles, so some workgroups take a second tile."""
import gzip
import json
import logging
import os
import struct
import zlib

import numpy as np
import pytest

from ribodetector_amd import _native as N
from ribodetector_amd import bam

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
FILL = 0xA5


# ---- chunks built by hand --------------------------------------------------------------------------------------------------------------
def _chunk(records, fasta=False):
    """(text bytes, rec_start, seq_off, seq_len) of records [(header line without '@', seq, qual or None, plus line)]"""
    parts, rs, so, sl, at = [], [0], [], [], 0
    for rec in records:
        head, seq, qual = rec[0], rec[1], rec[2]
        plus = rec[3] if len(rec) > 3 else b"+"
        t = (b">" if fasta else b"@") + head + b"\n"
        so.append(at + len(t))
        sl.append(len(seq))
        t += seq + b"\n"
        if not fasta:
            t += plus + b"\n" + qual + b"\n"
        parts.append(t)
        at += len(t)
        rs.append(at)
    return b"".join(parts), np.asarray(rs, np.int64), np.asarray(so, np.int64), np.asarray(sl, np.int32)


def _encode(text, rs, so, sl, n, flags, raw_cap=None, first=0, stride=1):
    """one call on the device; returns (raw buffer with its guard as numpy, raw_start, info)"""
    import torch
    from ribodetector_amd import ubam
    fasta = bool(flags & N.UBAM_FASTA)
    cap = bam.ubam_bound(len(text), n, fasta) if raw_cap is None else raw_cap
    raw = torch.full((((cap + 15) // 16) * 16 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV) if len(text) else torch.zeros(16, dtype=torch.uint8, device=DEV)
    tabs = [torch.from_numpy(x).to(DEV) for x in (rs, so, sl)]
    _, raw_start, info = ubam.encode(t, *tabs, n, flags, raw_cap=cap, raw=raw, rec_first=first, rec_stride=stride, text_bytes=len(text))
    torch.cuda.synchronize()
    return raw.cpu().numpy(), raw_start.cpu().numpy(), info.cpu().numpy()


def _check(records, n_mates=1, mate=0, fasta=False, counts=True):
    """encode the records and hold everything against bam.from_fastq of their text"""
    from ribodetector_amd import ubam
    text, rs, so, sl = _chunk(records, fasta)
    n = len(records)
    want = bam.from_fastq(text, n_mates, mate, fasta)
    sizes = [struct.unpack_from("<i", want, 0)[0] + 4] if n else []
    p = sizes[0] if n else 0
    while p < len(want):
        sizes.append(struct.unpack_from("<i", want, p)[0] + 4)
        p += sizes[-1]
    assert len(sizes) == n
    assert len(want) <= bam.ubam_bound(len(text), n, fasta)
    got, raw_start, info = _encode(text, rs, so, sl, n, ubam.flags_word(n_mates, mate, fasta))
    assert info[3] == 0 and info[0] == n and info[1] == len(want) and info[2] == -1 and info[7] == -1, info
    assert np.array_equal(raw_start, np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64))
    if got[:len(want)].tobytes() != want:
        bad = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
        raise AssertionError("raw differs at %d bytes, first %d last %d of %d" % (len(bad), bad[0], bad[-1], len(want)))
    assert (got[len(want):] == FILL).all(), "bytes written behind the records"
    if counts:
        c = bam.ubam_counts(text, n_mates, mate, fasta)
        assert (int(info[4]), int(info[5]), int(info[6])) == (c["bases_changed"], c["quals_clamped"], c["names_starred"]), (info, c)
    return want, raw_start


def _seq(rng, n, letters=b"ACGTN"):
    return bytes(rng.choice(np.frombuffer(letters, np.uint8), size=n)) if n else b""


def _qual(rng, n, lo=33, hi=74):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8)) if n else b""


def test_crafted_lengths_on_every_residue():
    rng = np.random.default_rng(1)
    records, k = [], 0
    for l_seq in (0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257):
        for l_name in (1, 2, 15, 16, 17, 254):
            name = bytes(rng.integers(65, 91, l_name, dtype=np.uint8))
            records.append((name + b" comment %d" % k, _seq(rng, l_seq, b"ACGTNacgtUuRY=."), _qual(rng, l_seq, 20, 140)))
            k += 1
    # the same records again behind fillers of 38 + t bytes: record starts on every residue modulo 16 of the output
    fillers = [(b"f", _seq(rng, t), _qual(rng, t)) for t in range(16)]
    mixed = []
    for i, r in enumerate(records):
        mixed += [fillers[i % 16], r, fillers[(3 * i + 1) % 16]]
    want, raw_start = _check(mixed)
    starts = {(int(s) % 16, len(m[1])) for s, m in zip(raw_start, mixed)}
    assert {s % 16 for s in raw_start[:-1].tolist()} == set(range(16))
    assert len({r for r, _ in starts}) == 16
    assert bam.fastq_text(want, 0).count(b"\n") == 4 * len(mixed)


def test_all_byte_values_as_bases_and_qualities():
    every = bytes(b for b in range(256) if b != 10)              # (a newline cannot stand inside a line)
    rec = (b"all", every * 2 + every[:37], (every * 2 + every[:37])[::-1])
    want, _ = _check([(b"a", b"AC", b"II"), rec, (b"b", b"", b"")])
    back = bam.fastq_text(want, 0).split(b"\n")
    assert back[5] == rec[1].translate(bam.UBAM_LETTER)
    assert back[7] == bytes(min(max(c, 33), 126) for c in rec[2])
    # the tables of the rule, through the device: one record per byte value, as its only base and as its only quality
    singles = [(b"v%d" % b, bytes([b]), bytes([b])) for b in range(256) if b != 10]
    want, raw_start = _check(singles)
    for k, (_, s, q) in enumerate(singles):
        r = want[raw_start[k]:raw_start[k + 1]]
        assert r[-2] >> 4 == bam.UBAM_CODE[s[0]] and r[-2] & 15 == 0 and r[-1] == bam.UBAM_QUAL[q[0]]


def _sweep_records(n, seed, longest=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, n)
    pool_s, pool_q = _seq(rng, 1 << 16, b"ACGTACGTACGTNacgtu"), _qual(rng, 1 << 16, 30, 130).replace(b"\n", b"I")
    out = []
    for i, ls in enumerate(lens.tolist()):
        a = int(rng.integers(0, (1 << 16) - longest))
        head = b"r%d" % i + (b"/1" if i % 7 == 0 else b"/2" if i % 11 == 0 else b"") + (b" c" if i % 5 == 0 else b"\tx" if i % 13 == 0 else b"")
        out.append((head, pool_s[a:a + ls], pool_q[a:a + ls], b"+" + (b"r%d" % i if i % 17 == 0 else b"")))
    return out


def test_sweep_of_70000_records():
    records = _sweep_records(70000, 2)
    want, raw_start = _check(records)
    assert len(want) > 1024 * 16384, "the write pass must take a second trip"
    _check(records[:5000], n_mates=2, mate=1)                    # /2 stripped, flag 141


def test_a_record_of_100000_bases_between_short_ones():
    rng = np.random.default_rng(3)
    short = [(b"s%d" % i, _seq(rng, 20 + i), _qual(rng, 20 + i)) for i in range(40)]
    big = (b"big one", _seq(rng, 100000, b"ACGTNacgt"), _qual(rng, 100000, 30, 130).replace(b"\n", b"#"))
    odd = (b"odd", _seq(rng, 99999), _qual(rng, 99999))
    _check(short[:20] + [big] + short[20:30] + [odd] + short[30:])


def test_interleaved_and_mate_files():
    rng = np.random.default_rng(4)
    records = []
    for i in range(3000):
        l1, l2 = int(rng.integers(0, 160)), int(rng.integers(0, 160))
        tail1, tail2 = ((b"/1", b"/2"), (b"", b""), (b"/2", b"/1"), (b"/1", b"/1"))[i % 4]
        records.append((b"p%d" % i + tail1 + b" 1:N", _seq(rng, l1), _qual(rng, l1)))
        records.append((b"p%d" % i + tail2, _seq(rng, l2), _qual(rng, l2)))
    records[10] = (b"/1", b"ACGT", b"IIII")                     # an id that is only /1: '*'
    records[11] = (b"/2 x", b"AC", b"II")
    want, raw_start = _check(records, n_mates=2, mate=bam.INTERLEAVED)
    recs = list(bam.records(want, 0))
    assert {r.flag for r in recs[0::2]} == {77} and {r.flag for r in recs[1::2]} == {141}
    assert recs[0].name == recs[1].name == b"p0" and recs[4].name == b"p2/2" and recs[5].name == b"p2/1" and recs[10].name == recs[11].name == b"*"
    for mate in (0, 1):
        want, _ = _check(records[mate::2], n_mates=2, mate=mate)
        assert {r.flag for r in bam.records(want, 0)} == {(77, 141)[mate]}
    _check(records, n_mates=1)                                   # single-end: /1 and /2 stay, flag 4
    # one mate of the interleaved chunk through rec_first / rec_stride
    from ribodetector_amd import ubam
    text, rs, so, sl = _chunk(records)
    for mate in (0, 1):
        want = bam.from_fastq(_chunk(records[mate::2])[0], 2, mate)
        got, raw_start, info = _encode(text, rs, so, sl, len(records) // 2, ubam.flags_word(2, mate), first=mate, stride=2)
        assert info[3] == 0 and info[1] == len(want) and got[:len(want)].tobytes() == want and (got[len(want):] == FILL).all()


def test_fasta():
    rng = np.random.default_rng(5)
    records = [(b"s%d desc" % i, _seq(rng, int(rng.integers(1, 400)), b"ACGTNRYKM"), None) for i in range(5000)]
    records += [(b"", b"ACGT", None), (b"long", _seq(rng, 70001), None)]
    want, _ = _check(records, fasta=True)
    assert bam.fastq_text(want, 0).split(b"\n")[3] == b'"' * len(records[0][1])
    text = _chunk(records, True)[0]
    assert len(want) <= len(text) + (len(text) + 1) // 2 + 40 * len(records)


def test_the_first_of_three_names_that_are_too_long():
    from ribodetector_amd import ubam
    rng = np.random.default_rng(6)
    records = [(b"n%d" % i, _seq(rng, 50), _qual(rng, 50)) for i in range(10000)]
    for i, extra in ((7777, 300), (4321, 255), (9000, 1000)):
        records[i] = (b"x" * extra + b" c", records[i][1], records[i][2])
    records[2000] = (b"ok" * 127, records[2000][1], records[2000][2])          # 254 bytes: fits
    records[6000] = (b"m", b"ACGTACGT", b"IIII")                              # a quality line shorter than its sequence
    records[5000] = (b"m", b"ACGT", b"IIIIIIII")                              # ... and longer
    text, rs, so, sl = _chunk(records)
    got, raw_start, info = _encode(text, rs, so, sl, len(records), ubam.flags_word())
    assert info[3] == 0 and info[2] == 4321 and info[7] == 5000, info
    assert (got[int(info[1]):] == FILL).all()
    with pytest.raises(ValueError, match="record 4321 is longer than 254"):
        bam.from_fastq(text)
    # the records in front of the first one are the rule's
    head = bam.from_fastq(_chunk(records[:4321])[0])
    assert got[:len(head)].tobytes() == head and raw_start[4321] == len(head)


def test_raw_cap_one_byte_short():
    from ribodetector_amd import ubam
    records = _sweep_records(3000, 7)
    text, rs, so, sl = _chunk(records)
    want = bam.from_fastq(text)
    for cap, fits in ((len(want), True), (len(want) - 1, False)):
        got, raw_start, info = _encode(text, rs, so, sl, len(records), ubam.flags_word(), raw_cap=cap)
        if fits:
            assert info[3] == 0 and got[:cap].tobytes() == want and (got[cap:] == FILL).all()
        else:
            assert info[3] == 1 and info[0] == 0 and info[1] == 0
            assert (got == FILL).all(), "written although the records do not fit"
            assert (raw_start == 0).all()
    # tables that do not describe the text: a status, nothing written
    bad = so.copy()
    bad[100] = len(text) + 5
    got, raw_start, info = _encode(text, rs, bad, sl, len(records), ubam.flags_word())
    assert info[3] == 2 and (got == FILL).all() and (raw_start == 0).all()
    # no records
    got, raw_start, info = _encode(b"", np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), 0, ubam.flags_word())
    assert info.tolist() == [0, 0, -1, 0, 0, 0, 0, -1] and raw_start.tolist() == [0] and (got == FILL).all()
    assert N.lib().rd_bam_encode(None, 0, None, None, None, 0, 0, 1, 1 << 30, None, 0, None, None, None, 0, None) != 0      # an unknown flag bit


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
SMALL = ["--chunk_size", "1", "-m", "3"]


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


def _read(path):
    with (gzip.open if path.endswith("gz") else open)(path, "rb") as fh:
        return fh.read()


def _inflate_bam(path):
    """the inflated bytes of a BGZF file, member by member; every member at most 65,280 bytes, the last one BGZF's end-of-file member"""
    data = open(path, "rb").read()
    assert data[-28:] == bam.EOF_MEMBER
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04" and data[p + 12:p + 16] == b"BC\x02\0"
        size = struct.unpack_from("<H", data, p + 16)[0] + 1
        d = zlib.decompressobj(31)
        piece = d.decompress(data[p:p + size])
        assert d.eof and not d.unused_data and len(piece) <= 65280
        out.append(piece)
        p += size
    assert p == len(data) and out[-1] == b""
    return b"".join(out)


HEADER = bam.encode_header((), bam.UBAM_HEADER_TEXT)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a few thousand synthetic reads, written with what the flag has to deal with: comments, /1 and /2, lower case, qualities"""
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("ubam")
    out = {}

    def write(path, arena, off, mate, fasta=False):
        raw, rng = arena.tobytes(), np.random.default_rng(len(off) + mate)
        with (gzip.open if path.endswith("gz") else open)(path, "wb") as fh:
            for i in range(len(off) - 1):
                s = raw[off[i]:off[i + 1]]
                if i % 9 == 0:
                    s = s[:len(s) // 2].lower() + s[len(s) // 2:]
                head = b"syn.%d" % i + (b"/%d" % mate if mate and i % 3 else b"") + (b" 1:N:0 x" if i % 2 else b"")
                if fasta:
                    fh.write(b">" + head + b"\n" + s + b"\n")
                else:
                    q = bytes(rng.integers(33, 75, len(s), dtype=np.uint8)) if i % 50 else b"\x7f" * len(s)
                    fh.write(b"@" + head + b"\n" + s + b"\n+\n" + q + b"\n")
        return path
    a, o, _ = synth.reads_numpy(3000, (60, 120), seed=41, rrna_frac=0.3)
    out["se"] = write(str(d / "se.fq"), a, o, 0)
    out["fa"] = write(str(d / "se.fa"), a, o, 0, fasta=True)
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(1500, (60, 120), seed=32, rrna_frac=0.3), synth.reads_numpy(1500, (60, 120), seed=33, rrna_frac=0.3)
    out["m1"], out["m2"] = write(str(d / "m1.fq.gz"), a1, o1, 1), write(str(d / "m2.fq.gz"), a2, o2, 2)
    with open(str(d / "il.fq"), "wb") as fh:
        r1, r2 = _read(out["m1"]).split(b"\n"), _read(out["m2"]).split(b"\n")
        for k in range(0, len(r1) - 1, 4):
            fh.write(b"\n".join(r1[k:k + 4] + r2[k:k + 4]) + b"\n")
    out["il"] = str(d / "il.fq")
    return out


def _both_runs(caplog, tmp_path, inputs, outs, extra=(), env=None, fasta=False, mates=None, unclassified=False):
    """the same command without the flag and with it; returns the flagged run and {name: (text of the plain run, BAM bytes)}"""
    n_mates = 1 if mates is None else 2
    res = {}
    for flag in (False, True):
        d = tmp_path / ("ubam" if flag else "text")
        d.mkdir()
        ext = ".bam" if flag else (".fa" if fasta else ".fq")
        o, r = [str(d / ("o%d%s" % (k, ext))) for k in range(outs)], [str(d / ("r%d%s" % (k, ext))) for k in range(outs)]
        rep, summ = str(d / "rep.tsv"), str(d / "summary.json")
        caplog.clear()
        with caplog.at_level(logging.INFO):
            p = _run(["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "--read_report", rep, "--summary", summ, *extra] +
                     (["--ubam_output"] if flag else []) + SMALL, env)
        files = {os.path.basename(x)[:2]: x for x in o + r}
        if unclassified:
            files.update({"u%d" % k: x + (".unclassified.bam" if flag else ".unclassified.gz") for k, x in enumerate(o)})
        res[flag] = (p, files, open(rep, "rb").read(), open(summ, "rb").read(), caplog.text, d)
    (p0, f0, rep0, raw0, log0, _), (p1, f1, rep1, raw1, log1, d1) = res[False], res[True]
    assert "names starred" not in log0
    assert all(v["path"] == "device" for v in p1.ingest.values())
    assert (p0.num_read, p0.num_nonrrna, p0.num_rrna, p0.num_unknown) == (p1.num_read, p1.num_nonrrna, p1.num_rrna, p1.num_unknown)
    # the summary: the new object is the last key, and the file without it is the plain run's, byte for byte
    s1 = json.loads(raw1)
    got = s1["ubam_output"]
    assert list(s1)[-1] == "ubam_output" and "ubam_output" not in json.loads(raw0)
    cut = raw1.index(b',\n "ubam_output": ')
    assert raw1[:cut] + b"\n}\n" == raw0, "the summary minus the new key is the same bytes"
    assert rep0 == rep1, "the report sees the FASTQ view"
    pairs = {}
    for key in f0:
        text = _read(f0[key])
        k = int(key[1])
        mate = 0 if mates is None else bam.INTERLEAVED if mates == "interleaved" and outs == 1 else k
        data = _inflate_bam(f1[key])
        assert data == HEADER + bam.from_fastq(text, n_mates, mate, fasta), key
        # the rule reads the output back to the guarantee's text, and so does this build's own -i path, for every file of the case
        assert bam.fastq_text(data) == _guarantee(text, n_mates, mate, fasta)
        _reads_back(d1 / ("again_" + key), f1[key], text, n_mates, mate, fasta)
        pairs[key] = (text, f1[key])
    return p1, pairs, got, log1


def _guarantee(text, n_mates, mate, fasta):
    out = []
    for k, (head, seq, qual) in enumerate(bam._text_records(text, fasta)):
        m = (k & 1) if mate == bam.INTERLEAVED else mate
        q = b'"' * len(seq) if qual is None else bytes(min(max(c, 33), 126) for c in qual)
        out.append(b"@" + bam.ubam_name(head, n_mates, m) + b"\n" + seq.translate(bam.UBAM_LETTER) + b"\n+\n" + q + b"\n")
    return b"".join(out)


def _counted(paths, n_mates, mates, fasta=False):
    tot = dict.fromkeys(("bases_changed", "quals_clamped", "names_starred"), 0)
    for path, mate in zip(paths, mates):
        for k, v in bam.ubam_counts(_read(path), n_mates, mate, fasta).items():
            tot[k] += v
    return tot


def _check_counters(got, log, want):
    assert got == want
    assert "%d bases changed, %d qualities clamped, %d names starred" % (want["bases_changed"], want["quals_clamped"], want["names_starred"]) in log


def _reads_back(d, path, text, n_mates, mate, fasta=False):
    """-i non.bam -o again.fq of this build (a single-end run over the one file, into the folder d): the guarantee's text, both
    classes together"""
    d.mkdir()
    o, r = str(d / "o.fq"), str(d / "r.fq")
    _run(["-l", "100", "-i", path, "-o", o, "-r", r] + SMALL)
    want = _guarantee(text, n_mates, mate, fasta)
    recs = lambda t: sorted(b"\n".join(x) for x in zip(*[iter(t.split(b"\n")[:-1])] * 4))     # noqa: E731
    assert recs(_read(o) + _read(r)) == recs(want)


def test_cli_single_end_plain(tmp_path, inputs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["se"]], 1)
    assert p.num_read == 3000 and min(len(t) for t, _ in pairs.values()) > 0
    _check_counters(got, log, _counted([inputs["se"]], 1, [0]))
    assert got["bases_changed"] > 0 and got["quals_clamped"] > 0


def test_cli_two_files_gz(tmp_path, inputs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["m1"], inputs["m2"]], 2, extra=["-e", "rrna"], mates="files")
    assert p.is_paired and p.num_read == 1500 and len(pairs) == 4
    _check_counters(got, log, _counted([inputs["m1"], inputs["m2"]], 2, [0, 1]))
    n1, n2 = [[r.name for r in bam.records(_inflate_bam(pairs[k][1]))] for k in ("o0", "o1")]
    assert n1 == n2 and len(n1) == p.num_nonrrna, "the mates share a QNAME"


@pytest.mark.parametrize("outs", [1, 2])
def test_cli_interleaved(tmp_path, inputs, outs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["il"]], outs, extra=["--interleaved"], mates="interleaved")
    assert p.num_read == 1500
    _check_counters(got, log, _counted([inputs["il"]], 2, [bam.INTERLEAVED]))
    recs = list(bam.records(_inflate_bam(pairs["o0"][1])))
    if outs == 1:
        assert len(recs) == 2 * p.num_nonrrna and all(a.name == b.name and (a.flag, b.flag) == (77, 141) for a, b in zip(recs[0::2], recs[1::2]))
    else:
        assert len(recs) == p.num_nonrrna and {r.flag for r in recs} == {77}


def test_cli_ensure_both(tmp_path, inputs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["m1"], inputs["m2"]], 2, extra=["-e", "both"], mates="files", unclassified=True)
    assert set(pairs) == {"o0", "o1", "r0", "r1", "u0", "u1"}
    assert sum(1 for _ in bam.records(_inflate_bam(pairs["u0"][1]))) == p.num_unknown
    _check_counters(got, log, _counted([inputs["m1"], inputs["m2"]], 2, [0, 1]))


def test_cli_fasta(tmp_path, inputs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["fa"]], 1, fasta=True)
    assert p.num_read == 3000
    # (the chunk's text is the FASTA view, upper-cased by the reader: what the plain run writes is what is counted)
    want = dict.fromkeys(("bases_changed", "quals_clamped", "names_starred"), 0)
    for text, _ in pairs.values():
        for k, v in bam.ubam_counts(text, 1, 0, True).items():
            want[k] += v
    _check_counters(got, log, want)
    assert all(r.qual == b"\xff" * len(r.qual) for r in bam.records(_inflate_bam(pairs["o0"][1])))


def test_cli_host_deflate(tmp_path, inputs, caplog):
    p, pairs, got, log = _both_runs(caplog, tmp_path, [inputs["se"]], 1, env={"RD_DEVICE_GZIP": "host"})
    _check_counters(got, log, _counted([inputs["se"]], 1, [0]))


def test_cli_a_name_that_is_too_long(tmp_path, inputs):
    lines = _read(inputs["se"]).split(b"\n")
    lines[4 * 1500] = b"@" + b"y" * 300 + b" c"
    bad = str(tmp_path / "bad.fq")
    open(bad, "wb").write(b"\n".join(lines))
    o, r = str(tmp_path / "o.bam"), str(tmp_path / "r.bam")
    with pytest.raises(ValueError, match="--ubam_output: the name of record 1500 is longer than 254 bytes"):
        _run(["-l", "100", "-i", bad, "-o", o, "-r", r, "--ubam_output"] + SMALL)
    # (chunks of 1,024 records) the chunk in front of the failing one is in the outputs, whole files both
    names = [rec.name for path in (o, r) for rec in bam.records(_inflate_bam(path))]
    assert len(names) == 1024 and set(names) == {b"syn.%d" % i for i in range(1024)}


def test_cli_input_without_a_final_newline(tmp_path, inputs):
    """the last line of a file may lack its '\\n': the chunk has it all the same, and the last record is a BAM record like the others"""
    text = b"\n".join(_read(inputs["se"]).split(b"\n")[:4 * 700])
    assert not text.endswith(b"\n")
    src = str(tmp_path / "cut.fq")
    open(src, "wb").write(text)
    o, r = str(tmp_path / "o.bam"), str(tmp_path / "r.bam")
    p = _run(["-l", "100", "-i", src, "-o", o, "-r", r, "--ubam_output"] + SMALL)
    assert p.num_read == 700
    data = b"".join(_inflate_bam(path)[len(HEADER):] for path in (o, r))
    want = bam.from_fastq(text + b"\n")
    cut = lambda d: sorted(d[rec.offset:rec.offset + rec.size] for rec in bam.records(d, 0))     # noqa: E731
    assert len(data) == len(want) and cut(data) == cut(want)
    assert any(rec.name == b"syn.699" for rec in bam.records(data, 0))


def test_cli_no_record_selected(tmp_path):
    empty = str(tmp_path / "empty.fq")
    open(empty, "wb").close()
    o, r = str(tmp_path / "o.bam"), str(tmp_path / "r.bam")
    _run(["-l", "100", "-i", empty, "-o", o, "-r", r, "--ubam_output"] + SMALL)
    for path in (o, r):
        assert _inflate_bam(path) == HEADER
        assert open(path, "rb").read()[-28:] == bam.EOF_MEMBER and len(open(path, "rb").read()) < 28 + 120
