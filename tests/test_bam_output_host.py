"""--bam_output without a GPU: the rule (bam.select / bam.header), the argument rules that hold before anything touches a device, and
the host writer's BAM mode (BGZF members and the end-of-file member for a name that ends in .bam / .ubam)."""
import gzip
import struct

import numpy as np
import pytest

from ribodetector_amd import bam, detect
from ribodetector_amd.data_loader import fastx_parser as fx


def _reads():
    """tags of several types, skipped records (first, last and runs of them), records without bases, a reverse-strand record"""
    rng = np.random.default_rng(5)
    out = []
    for i in range(60):
        n = int(rng.integers(0, 50)) if i % 7 else 0
        r = dict(name=b"r%d" % i, seq=bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)), qual=bytes(rng.integers(0, 60, n, dtype=np.uint8)))
        if i % 3 == 0:
            ml = bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))
            r["tags"] = b"MMZC+m,1,2;\0" + b"MLBC" + struct.pack("<i", len(ml)) + ml + b"XXZ" + b"x" * int(rng.integers(0, 20)) + b"\0"
        if i in (0, 59) or i % 10 in (4, 5):
            r.update(flag=0x100 if i % 2 else 0x800, ref_id=0, pos=3, cigar=[(n, "M")] if n else [])
        elif i % 5 == 0:
            r["flag"] = 0x10
        out.append(r)
    return out


def test_select_and_header_are_the_bytes_of_the_file(tmp_path):
    reads = _reads()
    text = b"@HD\tVN:1.6\tSO:unsorted\n@CO\tan input of its own\n"
    for tag, kw in (("one", {}), ("many", dict(member_bytes=[5, 1, 0, 40, 700]))):          # (the header inside one member, and across several)
        path = str(tmp_path / (tag + ".bam"))
        data = bam.write_bam(path, reads, refs=[(b"chr1", 1000)], text=text, **kw)
        n_hdr = bam.header_len(data)
        assert bam.header(path) == data[:n_hdr] and n_hdr == bam.header_bytes(path)
        recs = list(bam.records(data))
        kept = [r for r in recs if not r.skipped]
        assert len(recs) == 60 and 0 < len(kept) < 60 and recs[0].skipped and recs[-1].skipped and any(len(r.codes) == 0 for r in kept)
        every = bam.select(data, range(len(kept)))
        assert every == b"".join(bam.encode_record(r) for r in reads if not r.get("flag", 0) & 0x900)
        assert every == b"".join(data[r.offset:r.offset + r.size] for r in kept)
        keep = [0, 3, 4, len(kept) - 1]
        assert bam.select(data, keep) == b"".join(data[kept[k].offset:kept[k].offset + kept[k].size] for k in keep)
        assert bam.select(data, []) == b"" and bam.select(data, [len(kept)]) == b""
        assert bam.select(data[n_hdr:], keep, start=0) == bam.select(data, keep)
        # the selection behind the header is a BAM payload again, and its text is the text of the kept records
        assert bam.fastq_text(data[:n_hdr] + bam.select(data, keep)) == b"".join(kept[k].fastq() for k in keep)
    raw = bam.bgzf_member(b"BAM\2" + bytes(20)) + bam.EOF_MEMBER
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(raw)
    with pytest.raises(ValueError, match="not a BAM file"):
        bam.header(bad)


def test_argument_rules():
    words = "checked before anything touches a device"
    assert detect.check_bam(["a.bam"], ["o.bam"], None, True) is True
    assert detect.check_bam(["a.ubam", "b.bam"], ["o1.bam", "o2.ubam"], ["r1.bam", "r2.bam"], bam_output=True) is True
    for inputs, output, rrna in ((["a.fq"], ["o.bam"], None), (["a.bam", "b.fq"], ["o.bam", "p.bam"], None), (["a.fa"], ["o.bam"], None),
                                 (["a.bam"], ["o.fq"], None), (["a.bam"], ["o.fq.gz"], None), (["a.bam"], ["o.bam"], ["r.fq"]),
                                 (["a.bam", "b.bam"], ["o.bam", "p.fastq"], None)):
        with pytest.raises(RuntimeError, match=words):
            detect.check_bam(inputs, output, rrna, True)
    # without the flag: every result of the three-argument call
    with pytest.raises(RuntimeError, match="BAM output is not supported"):
        detect.check_bam(["a.bam"], ["o.bam"], None)
    with pytest.raises(RuntimeError, match="BAM output is not supported"):
        detect.check_bam(["a.bam"], ["o.fq"], ["r.ubam"], False)
    assert detect.check_bam(["a.bam"], ["o.fq"], None) is True and detect.check_bam(["a.fq"], ["o.fq"], None) is False
    # the flag on the command line, and the name of the unclassified pairs' file
    args = detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.bam", "--bam_output"])
    assert args.bam_output is True
    assert detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.fq"]).bam_output is False
    assert detect.unclassified_path("o.bam", True) == "o.bam.unclassified.bam" and detect.unclassified_path("o.fq") == "o.fq.unclassified.gz"
    out = ["o1.bam", "o2.bam"]
    with pytest.raises(RuntimeError, match="unclassified pairs' output file"):
        detect.check_read_report("o2.bam.unclassified.bam", out, None, True, "both", bam_output=True)
    with pytest.raises(RuntimeError, match="unclassified pairs' output file"):
        detect.check_summary("o1.bam.unclassified.bam", out, None, True, "both", bam_output=True)
    with pytest.raises(RuntimeError, match="unclassified pairs' output file"):
        detect.check_regions("o1.bam.unclassified.bam", True, out, None, True, "both", bam_output=True)
    detect.check_read_report("o2.bam.unclassified.gz", out, None, True, "both", bam_output=True)      # (not a file of such a run)
    detect.check_read_report("o2.bam.unclassified.bam", out, None, True, "rrna", bam_output=True)     # (no such file without -e both)
    with pytest.raises(RuntimeError, match="unclassified pairs' output file"):
        detect.check_read_report("o2.bam.unclassified.gz", out, None, True, "both")
    # BAM names count as outputs deflated on the device
    assert detect.Predictor.gz_output_files(["o1.bam", "o2.ubam"], ["r1.bam", "r2.bam"], True, "both") == [(0, 1), (1, 1), (0, 0), (1, 0), (0, -1), (1, -1)]
    assert detect.Predictor.gz_output_files(["o.fq"], ["r.fq.gz"], False, "none") == [(0, 1)]


def _members(raw):
    """[(offset, size, inflated bytes)] of a file of BGZF members: every one must carry the 'BC' subfield"""
    out, p = [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 10:p + 12] == b"\x06\0" and raw[p + 12:p + 16] == b"BC\x02\0", p
        size = struct.unpack_from("<H", raw, p + 16)[0] + 1
        out.append((p, size, struct.unpack_from("<I", raw, p + size - 4)[0]))
        p += size
    assert p == len(raw)
    return out


@pytest.mark.parametrize("ext", [".bam", ".ubam"])
def test_the_writer_puts_bam_names_into_bgzf_mode(tmp_path, ext):
    import ctypes as C
    from ribodetector_amd import _native as N
    eof = (C.c_uint8 * 28)()
    assert N.lib().rd_gz_eof_block(eof, 28) == 28          # (runs on the host: the block the device path's files end with)
    assert bytes(eof) == bam.EOF_MEMBER
    hdr = bam.encode_header([(b"chr1", 1000)], b"@HD\tVN:1.6\n@CO\tx\n")
    path = str(tmp_path / ("x" + ext))
    w = fx.open_for_write(path)
    a = np.frombuffer(hdr, np.uint8)
    w.write_text(a.ctypes.data, a.size)
    w.close()
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == hdr
    mem = _members(raw)
    assert [m[2] for m in mem] == [len(hdr), 0]
    assert raw[-28:] == bam.EOF_MEMBER and raw.count(bam.EOF_MEMBER) == 1
    # nothing written: still a BGZF file, the end-of-file member alone
    w = fx.open_for_write(path)
    w.close()
    assert open(path, "rb").read() == bam.EOF_MEMBER
    # 300,000 bytes that do not compress, in pieces: members of at most 65,536 inflated bytes that fit their 16-bit size
    big = np.random.default_rng(1).integers(0, 256, 300000, dtype=np.uint8)
    w = fx.open_for_write(path)
    for lo in range(0, big.size, 70001):
        piece = big[lo:lo + 70001]
        w.write_text(piece.ctypes.data, piece.size)
    w.close()
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == big.tobytes()
    mem = _members(raw)
    assert all(m[2] <= 65536 for m in mem) and sum(m[2] for m in mem) == big.size and mem[-1][2] == 0
    assert raw[-28:] == bam.EOF_MEMBER and raw.count(bam.EOF_MEMBER) == 1
    # a .gz name keeps its own members (no 'BC' subfield): the BAM mode is by name
    gzp = str(tmp_path / "x.fq.gz")
    w = fx.open_for_write(gzp)
    w.write_text(a.ctypes.data, a.size)
    w.close()
    assert open(gzp, "rb").read()[12:14] == b"RD"
