"""--bam_output on the GPU, through the CLI. The statement every file is compared against is the rule's: an output file inflates to
bam.header(its input) + bam.select(the input's inflated bytes, the delivered records that went to that file). WHICH records went to a
file comes from a second run of the same input with FASTQ outputs - the read names in its files - which ties the new path to the labels
of the existing one. Every member of every output must be a BGZF member of at most 65,536 inflated bytes, the end-of-file member last."""
import gzip
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bam as G  # noqa: E402
import test_interleaved_host as H  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- inputs and checks ----------------------------------------------------------------------------------------------------------------
def _tagged(reads, rng, skipped=True):
    """the reads with seeded tags of varying length (XX:Z, MM:Z, ML:B:C) and, after every 9th, a secondary / supplementary copy of it"""
    out = []
    for i, r in enumerate(reads):
        r = dict(r)
        ml = bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))
        tags = b""
        if i % 4 != 3:
            tags += b"XXZ" + bytes(rng.integers(33, 127, int(rng.integers(0, 50)), dtype=np.uint8)) + b"\0"
        if i % 3 == 0:
            tags += b"MMZC+m," + b",".join(b"%d" % x for x in rng.integers(0, 9, len(ml))) + b";\0" + b"MLBC" + struct.pack("<i", len(ml)) + ml
        r["tags"] = tags
        out.append(r)
        if skipped and i % 9 == 4:
            out.append(dict(r, flag=r.get("flag", 4) | (0x100 if i % 2 else 0x800), ref_id=0, pos=11, cigar=[(len(r["seq"]), "M")]))
    return out


def _inflate(path):
    """the file's inflated bytes (gzip: CRC-32 and ISIZE of every member are checked), after a walk over its members: each carries the
    'BC' subfield and at most 65,536 inflated bytes, the end-of-file member occurs once, last"""
    raw = open(path, "rb").read()
    p, sizes = 0, []
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 12:p + 16] == b"BC\x02\0", (path, p)
        size = struct.unpack_from("<H", raw, p + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", raw, p + size - 4)[0])
        assert sizes[-1] <= 65536
        if sizes[-1] == 0:
            assert raw[p:p + size] == bam.EOF_MEMBER and p + size == len(raw), (path, "an empty member that is not the last one", p)
        p += size
    assert p == len(raw) and raw.endswith(bam.EOF_MEMBER) and sizes[-1] == 0 and sizes.count(0) == 1, path
    return gzip.decompress(raw)


def _names(fq_path):
    with (gzip.open if fq_path.endswith("gz") else open)(fq_path, "rb") as fh:
        return [ln[1:] for ln in fh.read().split(b"\n")[0::4] if ln]


def _is_selection(bam_out, fq_out, bam_in, data_in):
    """bam_out = header(bam_in) + the records of bam_in, as they stand, whose names are in fq_out - in input order. Returns their number"""
    delivered = [r for r in bam.records(data_in) if not r.skipped]
    index = {r.name: k for k, r in enumerate(delivered)}
    assert len(index) == len(delivered)
    keep = [index[n] for n in _names(fq_out)]
    assert keep == sorted(keep)
    got = _inflate(bam_out)
    hdr = bam.header(bam_in)
    assert got[:len(hdr)] == hdr == data_in[:bam.header_len(data_in)], bam_out
    assert got[len(hdr):] == bam.select(data_in, keep), bam_out
    assert bam.fastq_text(got) == b"".join(delivered[k].fastq() for k in keep)
    return len(keep)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("bamout")
    rng = np.random.default_rng(50)
    out = {"dir": d}

    def make(tag, reads, co, **kw):
        path = str(d / (tag + ".bam"))
        data = bam.write_bam(path, reads, text=b"@HD\tVN:1.6\tSO:unsorted\n@CO\t" + co + b"\n", **kw)
        return path, data
    a, o, _ = synth.reads_numpy(600, (60, 120), seed=51, rrna_frac=0.4)
    out["se_reads"] = _tagged(G._bam_reads(a, o, rng=rng), rng)
    out["se"] = make("se", out["se_reads"], b"single-end input")
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(600, (60, 120), seed=52, rrna_frac=0.4), synth.reads_numpy(600, (60, 120), seed=53, rrna_frac=0.4)
    r1, r2 = _tagged(G._bam_reads(a1, o1, mate=1, rng=rng), rng, skipped=False), _tagged(G._bam_reads(a2, o2, mate=2, rng=rng), rng, skipped=False)
    out["a"], out["b"] = make("a", r1, b"mate 1 of two files", refs=[(b"chr1", 1000)]), make("b", r2, b"mate 2 of two files")
    out["il"] = make("il", H.interleave(r1, r2), b"interleaved input")
    return out


def _run_pair(tmp_path, tag, inputs, outs, extra=(), env=None, both=False):
    """the run with --bam_output and the run with FASTQ outputs; returns ([(bam file, fastq file)] of every output, the BAM run)"""
    d = tmp_path / tag
    d.mkdir()
    o, r = [str(d / ("o%d" % k)) for k in range(outs)], [str(d / ("r%d" % k)) for k in range(outs)]
    pb = G._run(["-l", "100", "-i", *inputs, "-o", *[x + ".bam" for x in o], "-r", *[x + ".ubam" for x in r], "--bam_output", *extra] + G.SMALL, env)
    pf = G._run(["-l", "100", "-i", *inputs, "-o", *[x + ".fq" for x in o], "-r", *[x + ".fq.gz" for x in r], *extra] + G.SMALL)
    assert (pb.num_read, pb.num_nonrrna, pb.num_rrna, pb.num_unknown) == (pf.num_read, pf.num_nonrrna, pf.num_rrna, pf.num_unknown)
    files = [(x + ".bam", x + ".fq") for x in o] + [(x + ".ubam", x + ".fq.gz") for x in r]
    if both:
        files += [(x + ".bam.unclassified.bam", x + ".fq.unclassified.gz") for x in o]
        assert not any(os.path.exists(x + ".bam.unclassified.gz") for x in o)
    assert all(os.path.exists(b) and os.path.exists(f) for b, f in files)
    return files, pb


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def test_single_end(tmp_path, sets):
    from ribodetector_amd.data_loader import device_reader as dr
    path, data = sets["se"]
    recs = list(bam.records(data))
    delivered = [r for r in recs if not r.skipped]
    assert len(delivered) == 600 and len(recs) > 650                      # (the skipped records of the input)
    files, p = _run_pair(tmp_path, "se", [path], 1)
    assert p.num_read == 600 and min(p.num_nonrrna, p.num_rrna) > 50
    counts = [_is_selection(b, f, path, data) for b, f in files]
    assert counts == [p.num_nonrrna, p.num_rrna]
    # the two files' records merged by input offset are exactly the input's delivered records: none lost, none twice, none skipped
    hdr = bam.header_len(data)
    offset = {data[r.offset:r.offset + r.size]: r.offset for r in delivered}
    merged = []
    for b, _ in files:
        out = _inflate(b)
        merged += [offset[out[r.offset:r.offset + r.size]] for r in bam.records(out)]
        assert not any(r.skipped for r in bam.records(out))
    assert sorted(merged) == [r.offset for r in delivered] and hdr == bam.header_len(_inflate(files[0][0]))
    # the output is an input again: the device deflate's members through the device inflate, the text that of the FASTQ run
    non_bam, non_fq = files[0]
    text = b"".join(c.to_host()[0].tobytes() for c in dr.get_seq_chunks_device(non_bam, chunk_size=256, first_chunk=256, device=DEV))
    assert text == open(non_fq, "rb").read() == bam.fastq_text(_inflate(non_bam))
    # the device gzip off: rd_select_pack over the raw view, the host writer's BGZF members - the same inflated bytes
    files_h, _ = _run_pair(tmp_path, "se_host", [path], 1, env={"RD_DEVICE_GZIP": "host"})
    assert [_inflate(b) for b, _ in files_h] == [_inflate(b) for b, _ in files]


def test_two_files_ensure_both(tmp_path, sets):
    (pa, da), (pb_, db) = sets["a"], sets["b"]
    files, p = _run_pair(tmp_path, "pe", [pa, pb_], 2, extra=["-e", "both"], both=True)
    assert p.is_paired and p.num_read == 600 and p.num_unknown > 0
    for k, (b, f) in enumerate(files):                                      # (o0 o1 r0 r1 u0 u1: mate = k % 2)
        _is_selection(b, f, (pa, pb_)[k % 2], (da, db)[k % 2])
    assert b"mate 2 of two files" in _inflate(files[1][0])[:200] and b"mate 1 of two files" in _inflate(files[0][0])[:200]
    assert [os.path.basename(b) for b, _ in files[4:]] == ["o0.bam.unclassified.bam", "o1.bam.unclassified.bam"]


@pytest.mark.parametrize("outs", [1, 2])
def test_interleaved(tmp_path, sets, outs):
    path, data = sets["il"]
    files, p = _run_pair(tmp_path, "il%d" % outs, [path], outs, extra=["--interleaved", "-e", "both"], both=True)
    assert p.is_paired and p.num_read == 600
    n = [_is_selection(b, f, path, data) for b, f in files]
    assert sum(n) == 1200 and min(n) > 0
    assert all(b"interleaved input" in _inflate(b)[:200] for b, _ in files)


@pytest.fixture
def small_batches(monkeypatch):
    """call it: from then on one BGZF member per batch - batches end inside records, chunks are assembled from several pieces"""
    from ribodetector_amd.data_loader import device_reader as dr

    def apply():
        monkeypatch.setattr(dr.DeviceFeeder, "FIRST", 1 << 12)
        monkeypatch.setattr(dr.DeviceFeeder, "BATCH", 1 << 20)
        monkeypatch.setattr(dr.DeviceFeeder, "MAX_MEMBERS", 1)
    return apply


def test_batch_and_chunk_boundaries(tmp_path, sets, small_batches):
    """members of 5,001 inflated bytes, one per batch; chunks of 512 pairs: the outputs of the one-batch run, byte for byte inflated"""
    (pa, da), (pb_, db) = sets["a"], sets["b"]
    whole, pw = _run_pair(tmp_path, "whole", [pa, pb_], 2, extra=["-e", "both"], both=True)
    assert all(v["indexer"]["batches"] == 2 for v in pw.ingest.values())      # (the batch of the data and the empty one that ends a stream)
    small_batches()
    cut = []
    for tag, data in (("a", da), ("b", db)):
        path = str(tmp_path / (tag + "_cut.bam"))
        with open(path, "wb") as fh:
            for p in range(0, len(data), 5001):
                fh.write(bam.bgzf_member(data[p:p + 5001]))
            fh.write(bam.EOF_MEMBER)
        cut.append(path)
    files, p = _run_pair(tmp_path, "cut", cut, 2, extra=["-e", "both"], both=True)
    assert all(v["indexer"]["batches"] > 20 for v in p.ingest.values())
    assert [_inflate(b) for b, _ in files] == [_inflate(b) for b, _ in whole]


def test_the_reader_keeps_the_raw_records(tmp_path, sets, small_batches):
    """get_seq_chunks_device(keep_raw=True) under tiny batches and chunks of 16: chunk.raw is the rule's selection of the chunk's records,
    and the FASTQ side of the chunks is what it is without the flag"""
    from ribodetector_amd.data_loader import device_reader as dr
    path, data = sets["se"]
    small_batches()
    cut = str(tmp_path / "se_cut.bam")
    with open(cut, "wb") as fh:
        for p in range(0, len(data), 3001):
            fh.write(bam.bgzf_member(data[p:p + 3001]))
        fh.write(bam.EOF_MEMBER)
    plain = [c.to_host() for c in dr.get_seq_chunks_device(cut, chunk_size=16, first_chunk=16, device=DEV)]
    at = 0
    for k, c in enumerate(dr.get_seq_chunks_device(cut, chunk_size=16, first_chunk=16, device=DEV, keep_raw=True)):
        got = c.to_host()
        assert all(np.array_equal(x, y) for x, y in zip(got, plain[k]))
        raw, rs = c.raw[0].cpu().numpy(), c.raw[1].cpu().numpy()
        want = [bam.select(data, [i]) for i in range(at, at + c.n)]
        assert int(c.raw_total[0]) == int(rs[-1]) == sum(len(w) for w in want) and rs[0] == 0
        assert raw[:int(rs[-1])].tobytes() == b"".join(want) and np.array_equal(np.diff(rs), [len(w) for w in want])
        at += c.n
    assert at == 600 and k + 1 == len(plain)
    assert next(dr.get_seq_chunks_device(cut, chunk_size=16, first_chunk=16, device=DEV)).raw is None
    with pytest.raises(ValueError, match="keep_raw"):
        next(dr.get_seq_chunks_device(str(tmp_path / "x.fq"), device=DEV, keep_raw=True))


def test_an_empty_selection_and_an_empty_input(tmp_path, sets):
    """a file that receives no record is the header and the end-of-file member"""
    path, data = sets["se"]
    hdr = bam.header(path)
    empty = str(tmp_path / "none.bam")
    bam.write_bam(empty, [], text=b"@CO\tno records\n")
    o, r = str(tmp_path / "o.bam"), str(tmp_path / "r.bam")
    p = G._run(["-l", "100", "-i", empty, "-o", o, "-r", r, "--bam_output"] + G.SMALL)
    assert p.num_read == 0 and _inflate(o) == _inflate(r) == bam.header(empty) and b"no records" in _inflate(o)
    # only secondary / supplementary records behind one read: one file gets the read, the other nothing
    one = [sets["se_reads"][0]] + [dict(x, flag=0x100) for x in sets["se_reads"][1:40]]
    bam.write_bam(empty, one, text=b"@CO\tone read\n")
    p = G._run(["-l", "100", "-i", empty, "-o", o, "-r", r, "--bam_output"] + G.SMALL)
    assert p.num_read == 1
    got = sorted((_inflate(o), _inflate(r)), key=len)
    assert got[0] == bam.header(empty) and got[1] == bam.header(empty) + bam.encode_record(one[0])
    assert hdr != bam.header(empty)


def test_a_plain_gzip_member_as_input(tmp_path, sets):
    """no BGZF at all: the host zlib route into the same indexer - the same outputs"""
    path, data = sets["se"]
    files, _ = _run_pair(tmp_path, "bgzf", [path], 1)
    plain = str(tmp_path / "plain.bam")
    open(plain, "wb").write(gzip.compress(data[:40000], 6) + gzip.compress(data[40000:], 1))
    files_p, _ = _run_pair(tmp_path, "plain", [plain], 1)
    assert [_inflate(b) for b, _ in files_p] == [_inflate(b) for b, _ in files]


def test_without_the_flag_nothing_changes(tmp_path, sets):
    path, _ = sets["se"]
    with pytest.raises(RuntimeError, match="BAM output is not supported"):
        G._run(["-l", "100", "-i", path, "-o", str(tmp_path / "o.bam")] + G.SMALL)
    with pytest.raises(RuntimeError, match="checked before anything touches a device"):
        G._run(["-l", "100", "-i", path, "-o", str(tmp_path / "o.fq"), "--bam_output"] + G.SMALL)
