"""--ubam_tag_floats on the host: the rule (bam.tags_from_comment(floats=True), from_fastq, ubam_tag_counts) against the hand-written
case table of tests/ubam_tag_float_cases.py; floats=False is what it was; the text fixed point BAM -> tagged FASTQ -> BAM with float
tags (guarantee (a)); the rule of the flag and the summary's object."""
import struct

import pytest

import bam_float_cases as F
import bam_tags_cases as BT
import ubam_tag_float_cases as UF
import ubam_tags_cases as UT
from ribodetector_amd import bam

HEADER = bam.encode_header((), bam.UBAM_HEADER_TEXT)


@pytest.mark.parametrize("case", UF.CASES, ids=[c[0] for c in UF.CASES])
def test_the_rule_on_the_case_table(case):
    _, comment, names, _, _ = case
    line = UF.header(comment)
    assert bam.tags_from_comment(line, names, floats=True) == bam.tags_from_comment(line + b"\r\n", names, True) == UF.expected(case)
    # without the flag the float fields are counted and not looked at - unless another field makes the record malformed
    off = bam.tags_from_comment(line, names)
    listed = set()
    n_float = 0
    for field in comment.split(b"\t"):
        if field[:2] in names and field[:2] not in listed:
            listed.add(field[:2])
            n_float += field[3:4] == b"f" or field[3:6] == b"B:f"
    assert off[3] == (0 if off[2] else n_float)


def test_floats_off_is_what_it_was():
    for case in UT.CASES:
        assert bam.tags_from_comment(case[1], case[2]) == bam.tags_from_comment(case[1], case[2], floats=False) == UT.expected(case), case[0]
    text = b"".join(b"@r%d%s\nACGT\n+\nIIII\n" % (k, c[1][3:].split(b"\n")[0].replace(b"\r", b"")) for k, c in enumerate(UT.CASES) if c[1].startswith(b"@r1"))
    names = [b"XI", b"RG", b"MM", b"ML"]
    assert bam.from_fastq(text, tags=names, floats=False) == bam.from_fastq(text, tags=names)
    assert bam.ubam_tag_counts(text, names, floats=False) == bam.ubam_tag_counts(text, names)
    assert bam.ubam_tag_counts(text, names)["float_values_skipped"] > 0


def test_from_fastq_and_the_counters_over_the_table():
    names = [b"qs", b"XF", b"RG", b"NM", b"ML"]
    text = UF.fastq([(b"r%d" % k, c[1]) for k, c in enumerate(UF.CASES)])
    plain, tagged = bam.from_fastq(text), bam.from_fastq(text, tags=names, floats=True)
    a, b = list(bam.records(HEADER + plain)), list(bam.records(HEADER + tagged))
    want, copied = {"malformed_records": 0, "float_values_skipped": 0}, [0] * len(names)
    for x, y, head in zip(a, b, text.split(b"\n")[0::4]):
        tags, c, mal, fl = bam.tags_from_comment(head, names, floats=True)
        bx, by = (HEADER + plain)[x.offset:x.offset + x.size], (HEADER + tagged)[y.offset:y.offset + y.size]
        assert by[4:] == bx[4:] + tags and struct.unpack_from("<i", by)[0] == struct.unpack_from("<i", bx)[0] + len(tags)
        want["malformed_records"] += mal
        want["float_values_skipped"] += fl
        copied = [p + q for p, q in zip(copied, c)]
    got = bam.ubam_tag_counts(text, names, floats=True)
    assert got == dict(want, copied=copied)
    assert got["malformed_records"] >= 20 and got["float_values_skipped"] >= 6 and copied[0] >= 10 and copied[1] >= 4


def _originals():
    """BAM data whose names hold no white space: the well-formed records of tests/bam_tags_cases.py, random ones, and records with
    qs:f, rq:f and B:f arrays of 0, 1 and 300 elements - the hard patterns of the formatter among them, NaNs and infinities included"""
    recs = [r for what, r, want in BT.CASES if want != "malformed" and not what.startswith("decoy")] + BT.random_records(5, 300, damaged_every=10 ** 9)
    hard = F.hard()[:600] + F.NANS + F.randoms(9, 900)
    for k in range(0, 300):
        tags = F.f_tag(b"qs", hard[3 * k]) + BT.Z(b"RG", b"lib%d" % (k % 3)) + F.f_tag(b"rq", hard[3 * k + 1])
        tags += F.bf_tag(b"XF", [[], [hard[3 * k + 2]], hard[k:k + 300]][k % 3])
        recs.append(BT.rec(tags, name=b"f%d" % k))
    return HEADER + b"".join(recs)


@pytest.mark.parametrize("names", [[b"qs"], [b"XF", b"RG", b"rq", b"qs"],
                                   [b"RG", b"XA", b"XC", b"Xc", b"XS", b"Xs", b"XI", b"Xi", b"Xf", b"XZ", b"XH", b"qs", b"NM", b"ML", b"XF", b"rq"]],
                         ids=["qs", "four", "sixteen"])
def test_guarantee_a_text_fixed_point_with_floats(names):
    d = _originals()
    t = bam.fastq_text_tagged(d, names, floats=True)
    assert t.count(b":f:") >= 300 and b"nan" in t and b"-inf" in t
    back = HEADER + bam.from_fastq(t, tags=names, floats=True)
    assert bam.fastq_text_tagged(back, names, floats=True) == t
    assert bam.ubam_tag_counts(t, names, floats=True)["float_values_skipped"] == 0
    # a float that a %g text holds exactly comes back as its own bits; a NaN keeps its sign only
    n_same = 0
    for x, y in zip(bam.records(d), bam.records(back)):
        off, n, ty = bam.find_tag(d, x.offset, b"qs")
        if off >= 0 and ty == ord("f") and not bam.tag_comment(d, x.offset, names, True)[2]:
            v = struct.unpack("<I", d[off:off + 4])[0]
            off2, n2, ty2 = bam.find_tag(back, y.offset, b"qs")
            w = struct.unpack("<I", back[off2:off2 + 4])[0]
            assert ty2 == ord("f") and bam.float_g(w) == bam.float_g(v)
            n_same += w == v
    assert n_same > 50
    # without the new flag the way back leaves every float out, as it did
    assert bam.from_fastq(t, tags=names) != bam.from_fastq(t, tags=names, floats=True)
    assert bam.ubam_tag_counts(t, names)["float_values_skipped"] >= 300


def test_the_rule_of_the_flag(monkeypatch):
    from ribodetector_amd import detect
    monkeypatch.delenv("RD_DEVICE_PARSE", raising=False)
    monkeypatch.delenv("RD_INGEST", raising=False)
    on_device = lambda p: True      # noqa: E731
    assert detect.check_ubam(True, ["a.fq"], ["o.bam"], ["r.bam"], parse_wanted=on_device, ubam_tags="qs,RG", ubam_tag_floats=True) == [b"qs", b"RG"]
    assert detect.check_ubam_tags("qs", True, True) == [b"qs"] and detect.check_ubam_tags(None, True, False) is None
    with pytest.raises(RuntimeError, match="--ubam_tag_floats .* give --ubam_tags LIST with it .*before anything touches a device"):
        detect.check_ubam(True, ["a.fq"], ["o.bam"], None, parse_wanted=on_device, ubam_tag_floats=True)
    with pytest.raises(RuntimeError, match="--ubam_tag_floats .* give --ubam_tags LIST with it"):
        detect.check_ubam(False, ["a.fq"], ["o.fq"], None, ubam_tag_floats=True)
    parser = detect.build_parser()
    assert parser.parse_args(["-l", "100", "-i", "a.fq", "-o", "o.bam", "--ubam_output", "--ubam_tags", "qs", "--ubam_tag_floats"]).ubam_tag_floats is True
    assert parser.parse_args(["-l", "100", "-i", "a.fq", "-o", "o.bam", "--ubam_output", "--ubam_tags", "qs"]).ubam_tag_floats is False


def test_the_summary_object():
    from ribodetector_amd import ubam
    names = [b"qs", b"RG"]
    one = {"copied": [3, 5], "malformed_records": 1, "float_values_skipped": 2}
    two = {"copied": [4, 0], "malformed_records": 0, "float_values_skipped": 7}
    doc = ubam.to_json_tags(names, [one], floats=True)
    assert doc == {"tags": ["qs", "RG"], "copied": [3, 5], "malformed_records": 1, "float_values_skipped": 2, "float_rounding": "nearest-even"}
    assert list(doc)[-1] == "float_rounding" and list(ubam.to_json_tags(names, [one, two], floats=True))[-1] == "float_rounding"
    assert ubam.to_json_tags(names, [one, two], floats=False) == ubam.to_json_tags(names, [one, two])
    assert "float_rounding" not in ubam.to_json_tags(names, [one])
    assert ubam.log_line_tags(names, [one, two]) == "BAM tags from text: qs 7, RG 5 copied; 1 records with malformed tags, 9 float values skipped"
