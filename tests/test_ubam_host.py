"""--ubam_output without a GPU: the rule (bam.from_fastq, bam.ubam_name, bam.UBAM_HEADER_TEXT) held against bam.encode_record built by
hand, the guarantee of reading the records back, the size bounds, and the argument rules that hold before anything touches a device."""
import struct

import numpy as np
import pytest

from ribodetector_amd import bam, detect

CODES = bam.CODES


def _letter(c):
    """the rule for a base, stated again: the letter of CODES in either case, U as T, everything else N"""
    u = c - 32 if 97 <= c <= 122 else c
    return u if u in CODES else ord("T") if u == ord("U") else ord("N")


def _by_hand(head, seq, qual, flag, n_mates=1, mate=0):
    return bam.encode_record({"name": bam.ubam_name(head, n_mates, mate), "seq": bytes(_letter(c) for c in seq),
                              "qual": None if qual is None else bytes(min(max(c, 33), 126) - 33 for c in qual), "flag": flag})


def test_from_fastq_is_encode_record():
    rng = np.random.default_rng(1)
    recs = []
    for i in range(200):
        n = int(rng.integers(0, 70))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgtuURYKM=.x", np.uint8), size=n)) if n else b""
        qual = bytes(rng.integers(11, 200, n, dtype=np.uint8)).replace(b"\n", b"I").replace(b"\r", b"I") if n else b""
        recs.append((b"@read%d/%d some comment" % (i, 1 + i % 2), seq, qual))
    text = b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)
    for n_mates, mate, flag in ((1, 0, 4), (2, 0, 77), (2, 1, 141)):
        assert bam.from_fastq(text, n_mates, mate) == b"".join(_by_hand(h, s, q, flag, n_mates, mate) for h, s, q in recs)
    want = b"".join(_by_hand(h, s, q, (77, 141)[k & 1], 2, k & 1) for k, (h, s, q) in enumerate(recs))
    assert bam.from_fastq(text, 2, bam.INTERLEAVED) == want
    # fixed fields of one record, field by field
    one = bam.from_fastq(b"@q x\nACG\n+\nI!~\n")
    block, ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHIiii", one, 0)
    assert (block, ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen) == (len(one) - 4, -1, -1, 2, 0, 4680, 0, 4, 3, -1, -1, 0)
    assert one[36:] == b"q\0" + bytes([0x12, 0x40]) + bytes([40, 0, 93])           # no tags behind the qualities


def test_reading_back_gives_the_guarantee():
    text = b"@a/1 c\nacgtUuNx\n+a/1\n!\"I~\x7f\x01 J\n@b\n\n+\n\n@c\tz\nA\n+\n#\n"
    data = bam.encode_header((), bam.UBAM_HEADER_TEXT) + bam.from_fastq(text, 2, 0)
    assert [r.name for r in bam.records(data)] == [b"a", b"b", b"c"]
    assert bam.fastq_text(data) == b"@a\nACGTTTNN\n+\n!\"I~~!!J\n@b\n\n+\n\n@c\nA\n+\n#\n"
    # uppercase CODES letters and qualities in range: only the comment and the /1 are lost
    clean = b"@r9/1 1:N:0\nACGTNRYKM=\n+\nIIIIIIII!~\n"
    assert bam.fastq_text(bam.from_fastq(clean, 2, 0), 0) == b"@r9\nACGTNRYKM=\n+\nIIIIIIII!~\n"
    assert bam.fastq_text(bam.from_fastq(clean, 1, 0), 0) == b"@r9/1\nACGTNRYKM=\n+\nIIIIIIII!~\n"
    # (a c g t U u x: seven bases change, N stays; \x7f \x01 and the space: three qualities are clamped)
    assert bam.ubam_counts(text, 2, 0) == {"bases_changed": 7, "quals_clamped": 3, "names_starred": 0}


def test_the_base_map_on_all_256_values():
    for c in range(256):
        want = _letter(c)
        assert bam.UBAM_LETTER[c] == want and bam.UBAM_CODE[c] == CODES.index(want)
        if c != 10:
            rec = bam.from_fastq(b"@x\n" + bytes([c]) + b"\n+\nI\n")
            assert rec[-2] == CODES.index(want) << 4 and rec == _by_hand(b"@x", bytes([c]), b"I", 4)
    assert all(bam.UBAM_CODE[c] == i for i, c in enumerate(CODES)) and all(bam.UBAM_CODE[c + 32] == bam.UBAM_CODE[c] for c in b"ACMGRSVTWYHKDBN")
    assert bam.UBAM_CODE[ord("U")] == bam.UBAM_CODE[ord("u")] == 8 and bam.UBAM_CODE[ord("=")] == 0 and bam.UBAM_CODE[ord("X")] == 15


def test_the_quality_map_on_all_256_values():
    for c in range(256):
        want = min(max(c, 33), 126) - 33
        assert bam.UBAM_QUAL[c] == want
        if c != 10:
            assert bam.from_fastq(b"@x\nA\n+\n" + bytes([c]) + b"\n")[-1] == want
    assert bam.UBAM_QUAL[33] == 0 and bam.UBAM_QUAL[126] == 93 and bam.UBAM_QUAL[127] == 93 and bam.UBAM_QUAL[0] == 0


def test_the_name_rule():
    n = bam.ubam_name
    assert n(b"@id comment") == n(b"@id\tcomment") == n(b"@id\rx") == n(b"@id\vx") == n(b"@id\fx") == n(b"@id\n") == n(b">id") == b"id"
    assert n(b"@id/1") == b"id/1" and n(b"@id/2", 1, 0) == b"id/2"                       # single-end: kept
    assert n(b"@id/1", 2, 0) == b"id" and n(b"@id/2", 2, 1) == b"id"                     # the right mate
    assert n(b"@id/2", 2, 0) == b"id/2" and n(b"@id/1", 2, 1) == b"id/1"                 # the wrong mate: kept
    assert n(b"@id/1/1", 2, 0) == b"id/1" and n(b"@id/1 x/1", 2, 0) == b"id"
    assert n(b"@/1", 2, 0) == b"*" and n(b"@/1") == b"/1" and n(b"@/2 c", 2, 1) == b"*"
    assert n(b"@") == n(b"@ comment") == n(b"@\tx", 2, 1) == b"*"
    ok, long = b"n" * 254, b"n" * 255
    rec = bam.from_fastq(b"@" + ok + b" c\nAC\n+\nII\n")
    assert rec[12] == 255 and rec[36:36 + 255] == ok + b"\0"
    with pytest.raises(ValueError, match="--ubam_output: the name of record 1 is longer than 254 bytes"):
        bam.from_fastq(b"@a\nA\n+\nI\n@" + long + b"\nAC\n+\nII\n@" + long + b"\nA\n+\nI\n")
    assert len(bam.from_fastq(b"@" + ok + b"/1\nAC\n+\nII\n", 2, 0)) == 36 + 255 + 1 + 2          # 256 bytes, 254 behind the strip
    with pytest.raises(ValueError, match="quality line of record 0"):
        bam.from_fastq(b"@a\nAC\n+\nI\n")
    assert bam.ubam_counts(b"@\nA\n+\nI\n@/1\nA\n+\nI\n@*\nA\n+\nI\n", 2, 0)["names_starred"] == 2


def test_l_seq_0_1_2():
    for seq, qual, packed in ((b"", b"", b""), (b"C", b"5", b"\x20"), (b"CT", b"5~", b"\x28")):
        rec = bam.from_fastq(b"@r\n" + seq + b"\n+\n" + qual + b"\n")
        assert len(rec) == 36 + 2 + len(packed) + len(seq) and rec[38:38 + len(packed)] == packed
        assert rec == bam.encode_record({"name": b"r", "seq": seq, "qual": bytes(c - 33 for c in qual), "flag": 4})
        assert bam.fastq_text(rec, 0) == b"@r\n" + seq + b"\n+\n" + qual + b"\n"


def test_fasta():
    text = b">s1 desc\nACGT\nacgu\n>s2\nN\n>s3\n"
    data = bam.from_fastq(text, fasta=True)
    assert data == b"".join(bam.encode_record({"name": n, "seq": s, "qual": None, "flag": 4}) for n, s in ((b"s1", b"ACGTACGT"), (b"s2", b"N"), (b"s3", b"")))
    assert bam.fastq_text(data, 0) == b'@s1\nACGTACGT\n+\n""""""""\n@s2\nN\n+\n"\n@s3\n\n+\n\n'
    assert bam.ubam_counts(text, fasta=True) == {"bases_changed": 4, "quals_clamped": 0, "names_starred": 0}


def test_the_header():
    assert bam.UBAM_HEADER_TEXT == b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
    hdr = bam.encode_header((), bam.UBAM_HEADER_TEXT)
    assert hdr == b"BAM\1" + struct.pack("<i", 32) + b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + struct.pack("<i", 0)
    assert bam.header_len(hdr) == len(hdr) == 44 and list(bam.records(hdr)) == []


def test_the_size_bounds():
    # records without bases: the least text per record, the most bytes gained
    for fasta, texts in ((False, (b"@\n\n+\n\n", b"@a\n\n+\n\n", b"@ab c\n\n+\n\n")), (True, (b">\n\n", b">a\n\n", b">ab c\n\n"))):
        for t in texts:
            for k in (1, 7):
                assert len(bam.from_fastq(t * k, fasta=fasta)) <= bam.ubam_bound(len(t) * k, k, fasta)
    assert len(bam.from_fastq(b"@\n\n+\n\n")) == 6 + 32 == bam.ubam_bound(6, 1)          # FASTQ: the bound is met
    assert bam.ubam_bound(100, 3) == 196 and bam.ubam_bound(101, 3, True) == 101 + 51 + 120
    rng = np.random.default_rng(2)
    for fasta in (False, True):
        parts = []
        for i in range(3000):
            n = int(rng.integers(0, 40)) if i % 3 else int(rng.integers(0, 3))
            seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)) if n else b""
            head = (b"", b"x", b"/1", b"name%d" % i, b"name%d comment" % i)[int(rng.integers(0, 5))]
            parts.append(b">" + head + b"\n" + seq + b"\n" if fasta else b"@" + head + b"\n" + seq + b"\n+\n" + b"I" * n + b"\n")
            text = b"".join(parts) if i % 500 == 499 else None
            if text:
                for n_mates, mate in ((1, 0), (2, 0)):
                    assert len(bam.from_fastq(text, n_mates, mate, fasta)) <= bam.ubam_bound(len(text), i + 1, fasta)


def test_every_rule_of_check_ubam(monkeypatch):
    words = "checked before anything touches a device"
    on_device = lambda p: True                                                          # noqa: E731
    for k in ("RD_DEVICE_PARSE", "RD_INGEST", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    assert detect.check_ubam(False, ["a.bam"], ["o.fq"], None) is None                   # without the flag: nothing
    assert detect.check_ubam(True, ["a.fq"], ["o.bam"], ["r.ubam"], parse_wanted=on_device) is None
    assert detect.check_ubam(True, ["a.fa.gz", "b.fa.gz"], ["o.bam", "p.bam"], None, parse_wanted=on_device) is None
    with pytest.raises(RuntimeError, match="a.bam is a BAM file, whose records --bam_output writes.*" + words):
        detect.check_ubam(True, ["a.bam"], ["o.bam"], None, parse_wanted=on_device)
    with pytest.raises(RuntimeError, match="--bam_output.*give one of them.*" + words):
        detect.check_ubam(True, ["a.fq"], ["o.bam"], None, bam_output=True, parse_wanted=on_device)
    for o, r in ((["o.fq"], None), (["o.bam"], ["r.fq.gz"]), (["o.bam", "p.sam"], None)):
        with pytest.raises(RuntimeError, match="must end with .bam or .ubam - all outputs are BAM or none is.*" + words):
            detect.check_ubam(True, ["a.fq"] * len(o), o, r, parse_wanted=on_device)
    for env in ({"RD_DEVICE_PARSE": "0"}, {"RD_INGEST": "host"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            with pytest.raises(RuntimeError, match="RD_DEVICE_PARSE=0 or RD_INGEST=host.*" + words):
                detect.check_ubam(True, ["a.fq"], ["o.bam"], None, parse_wanted=on_device)
    with pytest.raises(RuntimeError, match="the text of a.fq.gz does not stay on the device.*" + words):
        detect.check_ubam(True, ["a.fq.gz"], ["o.bam"], None, parse_wanted=lambda p: False)
    with monkeypatch.context() as m:
        m.setenv("WORLD_SIZE", "2")
        with pytest.raises(RuntimeError, match="runs on one rank.*" + words):
            detect.check_ubam(True, ["a.fq"], ["o.bam"], None, parse_wanted=on_device)
    # the parser knows the flag, and main() applies the rules in front of the model
    args = detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.bam", "--ubam_output"])
    assert args.ubam_output is True
    with pytest.raises(RuntimeError, match="is a BAM file"):
        detect.main(["-l", "100", "-i", "a.bam", "-o", "o.bam", "--ubam_output"])
    assert detect.unclassified_path("o.bam", True) == "o.bam.unclassified.bam"


def test_check_bam_with_its_old_arguments(monkeypatch):
    for k in ("RD_DEVICE_PARSE", "RD_INGEST", "RD_DEVICE_INFLATE", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    assert detect.check_bam(["a.bam"], ["o.bam"], None, True) is True
    assert detect.check_bam(["a.bam"], ["o.fq"], None) is True and detect.check_bam(["a.fq"], ["o.fq"], None) is False
    with pytest.raises(RuntimeError, match="BAM output is not supported: o.bam"):
        detect.check_bam(["a.fq"], ["o.bam"], None)                                       # a .bam name without either flag
    with pytest.raises(RuntimeError, match="BAM output is not supported: r.ubam"):
        detect.check_bam(["a.fq"], ["o.fq"], ["r.ubam"], False, False, False)
    with pytest.raises(RuntimeError, match="every -i file must end with .bam or .ubam"):
        detect.check_bam(["a.fq"], ["o.bam"], None, True)
    assert detect.check_bam(["a.fq"], ["o.bam"], None, ubam_output=True) is False         # the new keyword: the names are the run's
