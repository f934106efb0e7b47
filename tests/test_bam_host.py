"""BAM input without a GPU: the format names, the rule of ribodetector_amd/bam.py (records, fastq_text) and its writer held to the
specification - a file built byte by byte here - the header length over several members, and the CLI's argument errors, which are
raised before anything touches a device. tests/test_gpu_bam.py compares the device against this rule."""
import gzip
import struct

import pytest

from ribodetector_amd import bam


def test_format_names():
    from ribodetector_amd.data_loader import fastx_parser as fx
    assert fx.get_seq_format("x.bam") == "bam" and fx.get_seq_format("/a/b/x.ubam") == "bam"
    assert fx.get_seq_format("x.fq.gz") == "fqgz" and fx.get_seq_format("x.fa") == "fa"
    with pytest.raises(ValueError, match="Unknown extension .sam. Only fastq and fasta sequence formats are supported"):
        fx.get_seq_format("x.sam")
    with pytest.raises(ValueError, match="Unknown extension"):
        fx.get_seq_format("x.bam.gz")
    from ribodetector_amd import _native as N
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ribodetector_amd.h")).read()
    assert int(re.search(r"#define RD_BAM_SEGMENT (\d+)", hdr).group(1)) == N.BAM_SEGMENT == bam.SEGMENT
    assert int(re.search(r"#define RD_BAM_RECORD (\d+)", hdr).group(1)) == N.BAM_RECORD
    assert int(re.search(r"#define RD_BAM_TRUNCATED (\d+)", hdr).group(1)) == N.BAM_TRUNCATED


def _inflate(path):
    return gzip.decompress(open(path, "rb").read())


def test_writer_is_pinned_to_the_specification(tmp_path):
    """one file built field by field from the layout table: a header with one reference, an unmapped record with an odd l_seq, a mapped
    one with a 2-op CIGAR on the reverse strand"""
    hdr = b"BAM\1" + struct.pack("<i", 12) + b"@HD\tVN:1.6\n\0" + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 1000)
    # record 1: name "r1", ACGTN (codes 1 2 4 8 15), quals 0 10 20 30 40, unmapped (flag 4), a tag XY:i:7 as 'C'
    body1 = (struct.pack("<ii", -1, -1) + struct.pack("<BBH", 3, 0, 4680) + struct.pack("<HH", 0, 4) + struct.pack("<I", 5) +
             struct.pack("<iii", -1, -1, 0) + b"r1\0" + bytes([0x12, 0x48, 0xF0]) + bytes([0, 10, 20, 30, 40]) + b"XYC\x07")
    # record 2: name "read/2", AACG (codes 1 1 2 4), quals 1 2 3 93, refID 0, pos 99, mapq 60, CIGAR 3M1S, flag 0x10
    body2 = (struct.pack("<ii", 0, 99) + struct.pack("<BBH", 7, 60, 4681) + struct.pack("<HH", 2, 0x10) + struct.pack("<I", 4) +
             struct.pack("<iii", -1, -1, 0) + b"read/2\0" + struct.pack("<II", (3 << 4) | 0, (1 << 4) | 4) + bytes([0x11, 0x24]) + bytes([1, 2, 3, 93]))
    by_hand = hdr + struct.pack("<i", len(body1)) + body1 + struct.pack("<i", len(body2)) + body2
    reads = [dict(name=b"r1", seq="ACGTN", qual=bytes([0, 10, 20, 30, 40]), tags=b"XYC\x07"),
             dict(name=b"read/2", seq="AACG", qual=bytes([1, 2, 3, 93]), flag=0x10, ref_id=0, pos=99, mapq=60, cigar=[(3, "M"), (1, "S")])]
    path = tmp_path / "two.bam"
    data = bam.write_bam(str(path), reads, refs=[(b"chr1", 1000)], text=b"@HD\tVN:1.6\n\0")
    assert data == by_hand and _inflate(path) == by_hand
    raw = open(path, "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:16] == b"BC\x02\x00" and raw.endswith(bam.EOF_MEMBER) and len(bam.EOF_MEMBER) == 28
    assert struct.unpack_from("<H", raw, 16)[0] + 1 == len(raw) - 28                  # BSIZE = the member's size - 1
    assert bam.header_len(by_hand) == len(hdr) == bam.header_bytes(str(path))
    recs = list(bam.records(by_hand))
    assert [(r.offset, r.size, r.name, r.flag) for r in recs] == [(len(hdr), 4 + len(body1), b"r1", 4), (len(hdr) + 4 + len(body1), 4 + len(body2), b"read/2", 0x10)]
    # the reverse-strand record: CGTT = reverse complement of AACG, qualities reversed
    assert bam.fastq_text(by_hand) == b"@r1\nACGTN\n+\n!+5?I\n" + b"@read/2\nCGTT\n+\n~$#\"\n"


def _text(read):
    return bam.fastq_text(bam.payload([read]))


def test_fastq_text_edges():
    for n in (0, 1, 2, 255):
        seq = ("ACGT" * 64)[:n]
        assert _text(dict(name=b"n", seq=seq, qual=bytes([30] * n))) == b"@n\n" + seq.encode() + b"\n+\n" + b"?" * n + b"\n"
        assert len(_text(dict(name=b"n", seq=seq, qual=bytes([30] * n)))) == 2 * n + 2 + 5
    codes = "=ACMGRSVTWYHKDBN"
    assert _text(dict(name=b"c", seq=codes, qual=bytes(range(16)))) == b"@c\n=ACMGRSVTWYHKDBN\n+\n" + bytes(range(33, 49)) + b"\n"
    assert _text(dict(name=b"c", seq=codes, qual=bytes(range(16)), flag=0x10)) == b"@c\nNVHMDRWABSYCKGT=\n+\n" + bytes(range(48, 32, -1)) + b"\n"
    # the complement of a code is its 4-bit bit reversal
    for c in range(16):
        assert bam.COMPLEMENT[c] == bam.CODES[int("{:04b}".format(c)[::-1], 2)]
    assert _text(dict(name=b"q", seq="AAAAA", qual=bytes([0, 93, 94, 254, 7]))) == b"@q\nAAAAA\n+\n!~~~(\n"
    assert _text(dict(name=b"q", seq="ACG", qual=None)) == b'@q\nACG\n+\n"""\n'
    assert _text(dict(name=b"q", seq="ACG", qual=None, flag=0x10)) == b'@q\nCGT\n+\n"""\n'
    assert _text(dict(name=b"q", seq="AC", qual=bytes([5, 0xFF]))) == b"@q\nAC\n+\n&~\n"          # (0xFF behind the first byte is a quality like any other)
    assert _text(dict(name=b"", seq="A", qual=b"\x01")) == b'@\nA\n+\n"\n'                         # l_read_name = 1: the NUL alone
    long_name = bytes(33 + i % 90 for i in range(254))
    assert _text(dict(name=long_name, seq="", qual=b"")) == b"@" + long_name + b"\n\n+\n\n"          # l_read_name = 255
    reads = [dict(name=b"a", seq="A", qual=b"\0"), dict(name=b"a", seq="C", qual=b"\0", flag=0x100), dict(name=b"a", seq="G", qual=b"\0", flag=0x800),
             dict(name=b"a", seq="T", qual=b"\0", flag=0x900 | 0x10), dict(name=b"b", seq="T", qual=b"\0", flag=0x400)]
    data = bam.payload(reads)
    assert [r.skipped for r in bam.records(data)] == [False, True, True, True, False]
    assert bam.fastq_text(data) == b"@a\nA\n+\n!\n@b\nT\n+\n!\n"


def test_walk_errors():
    good = [dict(name=b"g%d" % i, seq="ACGT", qual=b"\1\2\3\4") for i in range(3)]
    rec = bam.encode_record(good[0])

    def walk(tail):
        data = bam.payload(good) + tail
        out = []
        with pytest.raises(ValueError) as e:
            for r in bam.records(data):
                out.append(r.name)
        assert out == [b"g0", b"g1", b"g2"]
        return str(e.value)
    for block in (0, 31, -1):
        assert walk(struct.pack("<i", block) + rec[4:]) == "malformed BAM record 3"
    assert walk(struct.pack("<i", 0x7fffffff) + rec[4:]) == "truncated BAM record at end of file"
    assert walk(rec[:12] + b"\0" + rec[13:]) == "malformed BAM record 3"                           # l_read_name = 0
    assert walk(rec[:38] + b"x" + rec[39:]) == "malformed BAM record 3"                            # the name lost its NUL
    assert walk(rec[:20] + struct.pack("<I", 1000) + rec[24:]) == "malformed BAM record 3"         # l_seq larger than the record
    assert walk(rec[:-1]) == "truncated BAM record at end of file"
    assert walk(rec[:3]) == "truncated BAM record at end of file"
    with pytest.raises(ValueError, match="not a BAM file"):
        list(bam.records(b"BAM\2" + bytes(20)))
    with pytest.raises(ValueError, match="truncated BAM header"):
        list(bam.records(bam.encode_header([(b"chr1", 5)])[:-3]))


def test_header_bytes_inside_one_member_and_over_several(tmp_path):
    reads = [dict(name=b"r%d" % i, seq="ACGTACGT", qual=bytes(range(8))) for i in range(50)]
    p1 = tmp_path / "small.bam"
    bam.write_bam(str(p1), reads, refs=[(b"chr1", 10), (b"chrM", 20)], text=b"@HD\tVN:1.6\n")
    assert bam.header_bytes(str(p1)) == len(bam.encode_header([(b"chr1", 10), (b"chrM", 20)], b"@HD\tVN:1.6\n"))
    text = b"".join(b"@SQ\tSN:contig%06d\tLN:%d\n" % (i, 1000 + i) for i in range(7400))
    refs = [(b"contig%06d" % i, 1000 + i) for i in range(300)]
    assert len(text) > 200 << 10
    p2 = tmp_path / "big_header.bam"
    data = bam.write_bam(str(p2), reads, refs=refs, text=text)
    n = bam.header_bytes(str(p2))
    assert n == len(bam.encode_header(refs, text)) and n > 3 * 0xff00
    assert bam.fastq_text(data) == bam.fastq_text(data, start=n) == bam.fastq_text(bam.payload(reads))
    # members of other sizes inflate to the same bytes; an empty member is a member
    p3 = tmp_path / "members.bam"
    assert bam.write_bam(str(p3), reads, refs=refs, text=text, member_bytes=[1, 1, 0, 7, 0xff00], level=0) == data == _inflate(p3)
    assert bam.header_bytes(str(p3)) == n
    # damage: bad magic; a file that ends inside its header
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bam.bgzf_member(b"BAM\2" + data[4:2000]) + bam.EOF_MEMBER)
    with pytest.raises(ValueError, match="not a BAM file"):
        bam.header_bytes(str(bad))
    bad.write_bytes(bam.bgzf_member(data[:2000]) + bam.EOF_MEMBER)
    with pytest.raises(ValueError, match="truncated BAM header"):
        bam.header_bytes(str(bad))


BAD_ARGS = [
    (["-i", "a.bam", "-o", "o.bam"], {}, "BAM output is not supported"),
    (["-i", "a.fq", "-o", "o.fq", "-r", "r.ubam"], {}, "BAM output is not supported"),
    (["-i", "a.bam", "b.fq", "-o", "o1.fq", "o2.fq"], {}, "cannot be mixed with FASTQ / FASTA"),
    (["-i", "a.fa", "b.ubam", "-o", "o1.fq", "o2.fq"], {}, "cannot be mixed with FASTQ / FASTA"),
    (["-i", "a.bam", "-o", "o.fa"], {}, "written as FASTQ"),
    (["-i", "a.bam", "-o", "o.fq"], {"RD_DEVICE_PARSE": "0"}, "RD_DEVICE_PARSE=0"),
    (["-i", "a.bam", "-o", "o.fq.gz"], {"RD_DEVICE_INFLATE": "0"}, "RD_DEVICE_INFLATE=0"),
    (["-i", "a.bam", "-o", "o.fq"], {"RD_INGEST": "host"}, "on the device only"),
    (["-i", "a.bam", "-o", "o.fq"], {"WORLD_SIZE": "2"}, "runs on one rank"),
    (["--interleaved", "-i", "a.ubam", "-o", "o.fq"], {"WORLD_SIZE": "8"}, "runs on one rank"),
]


@pytest.mark.parametrize("argv,env,msg", BAD_ARGS)
def test_argument_errors_before_anything_touches_a_device(tmp_path, monkeypatch, argv, env, msg):
    from ribodetector_amd import detect
    for k in ("RD_DEVICE_PARSE", "RD_DEVICE_INFLATE", "RD_INGEST", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(detect.Predictor, "__init__", lambda self, *a, **k: pytest.fail("a Predictor was made"))
    monkeypatch.setattr(detect.Predictor, "load_model", lambda self: pytest.fail("the model was loaded"))
    argv = ["-l", "100"] + [a if a.startswith("-") else str(tmp_path / a) for a in argv]
    with pytest.raises(RuntimeError, match=msg) as e:
        detect.main(argv)
    assert "before anything touches a device" in str(e.value)


def test_arguments_accepted(tmp_path, monkeypatch):
    from ribodetector_amd import detect
    for k in ("RD_DEVICE_PARSE", "RD_DEVICE_INFLATE", "RD_INGEST", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    t = lambda name: str(tmp_path / name)      # noqa: E731
    assert detect.check_bam([t("a.bam")], [t("o.fq")], None) is True
    assert detect.check_bam([t("a.bam"), t("b.ubam")], [t("o1.fastq.gz"), t("o2.fq.gz")], [t("r1.fq"), t("r2.fq")]) is True
    assert detect.check_bam([t("a.fq")], [t("o.fq")], None) is False
    assert detect.check_bam([t("a.fa.gz")], [t("o.fa")], None) is False
    monkeypatch.setenv("RD_INGEST", "members")     # (members inflated on the device: what a BAM file consists of)
    assert detect.check_bam([t("a.bam")], [t("o.fq")], None) is True
    monkeypatch.setenv("WORLD_SIZE", "2")          # without a BAM input nothing changes
    assert detect.check_bam([t("a.fq")], [t("o.fq")], None) is False
    assert detect.check_file_counts([t("a.bam")], [t("o1.fq"), t("o2.fq")], None, interleaved=True) is True


def test_c_abi_argument_errors_without_gpu():
    """rd_bam_index / rd_bam_gather / rd_bam_sample share the checks of their FASTQ / FASTA siblings (tests/test_abi.py): refused before
    any HIP call, no pointer dereferenced - P / Q stand for an aligned / a misaligned one"""
    from ribodetector_amd import _native as N
    L = N.lib()
    P, Q, big = 0x10000, 0x10001, 1 << 40

    def refused(name, args, code, word):
        rc = getattr(L, name)(*args)
        msg = L.rd_last_error()
        assert rc == code and msg.startswith(name.encode() + b":") and word in msg, (name, args, rc, msg)

    def index(text=P, pad=64, end=4096, prev_text=None, prev=None, norm=P, norm_cap=1 << 16, cap_records=64, ws=P, ws_bytes=big):
        return (text, pad, end, prev_text, prev, 0, norm, norm_cap, P, P, cap_records, P, ws, ws_bytes, None)
    refused("rd_bam_index", index(text=None), -1, b"null")
    refused("rd_bam_index", index(norm=None), -1, b"null")
    refused("rd_bam_index", index(ws=None), -1, b"null")
    refused("rd_bam_index", index(end=63), -1, b"bad pad / end")
    refused("rd_bam_index", index(pad=-1), -1, b"bad pad / end")
    refused("rd_bam_index", index(end=0x7fffffff), -1, b"bad pad / end")
    refused("rd_bam_index", index(norm_cap=-1), -1, b"bad pad / end")
    refused("rd_bam_index", index(cap_records=0), -1, b"bad pad / end")
    refused("rd_bam_index", index(prev_text=P), -1, b"prev and prev_text go together")
    refused("rd_bam_index", index(prev=P), -1, b"prev and prev_text go together")
    refused("rd_bam_index", index(text=P + 32), -1, b"aligned")
    refused("rd_bam_index", index(ws=Q), -1, b"aligned")
    refused("rd_bam_index", index(norm=Q), -1, b"norm 16-byte aligned")
    refused("rd_bam_index", index(ws_bytes=0), -4, b"workspace too small")

    def gather(src=P, lo=0, hi=8, out=P, cur_out=P + 8):
        return (src, P, P, P, lo, hi, 4096, out, 4096, P, cur_out, P, P, P, None)
    refused("rd_bam_gather", gather(src=None), -1, b"null")
    refused("rd_bam_gather", gather(out=None), -1, b"null")
    refused("rd_bam_gather", gather(lo=9), -1, b"bad range")
    refused("rd_bam_gather", gather(cur_out=P), -1, b"bad range")
    refused("rd_bam_gather", gather(out=Q), -1, b"aligned")
    refused("rd_bam_sample", (None, P, 4096, P, 8, None), -1, b"bad argument")
    refused("rd_bam_sample", (P, P, 0, P, 8, None), -1, b"bad argument")
    # the workspace: per segment 32 bytes of results, a list of S / 37 + 1 eight-byte entries and three bases; 4 bytes per possible record
    S = bam.SEGMENT
    assert L.rd_bam_index_workspace_bytes(-1) == 0 and L.rd_bam_index_workspace_bytes(0x7fffffff) == 0
    a, b = L.rd_bam_index_workspace_bytes(0), L.rd_bam_index_workspace_bytes(100 * S)
    per_list = (S // 37 + 1) * 8
    assert a % 256 == 0 and per_list <= a < per_list + 8 * 256
    assert b % 256 == 0 and 101 * per_list + 4 * (100 * S // 37) <= b < 101 * (per_list + 48) + 4 * (100 * S // 37 + 2) + 8 * 256
