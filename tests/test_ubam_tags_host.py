"""--ubam_tags on the host: the rule (bam.tags_from_comment, from_fastq(tags=), ubam_tag_counts) against the hand-written case
table of tests/ubam_tags_cases.py, the text fixed point BAM -> tagged FASTQ -> BAM over the records of tests/bam_tags_cases.py, the
bound of the tag bytes, the rules of the flag and the summary's object."""
import random
import struct

import pytest

import bam_tags_cases as BT
import ubam_tags_cases as UT
from ribodetector_amd import bam

HEADER = bam.encode_header((), bam.UBAM_HEADER_TEXT)


@pytest.mark.parametrize("case", UT.CASES, ids=[c[0] for c in UT.CASES])
def test_the_rule_on_the_case_table(case):
    _, line, names, _, _, _ = case
    assert bam.tags_from_comment(line, names) == UT.expected(case)
    # the line with and without its end is the same line
    cut = line.split(b"\n")[0]
    assert bam.tags_from_comment(cut, names) == bam.tags_from_comment(cut + b"\n", names) == UT.expected(case)


def test_the_case_table_holds_what_the_issue_lists():
    ints = dict(UT.INT_EDGES)
    for text in (b"-2147483649", b"-2147483648", b"-32769", b"-32768", b"-129", b"-128", b"-1", b"0", b"255", b"256", b"65535", b"65536",
                 b"4294967295", b"4294967296", b"+5", b"007", b"12345678901", b"-", b""):
        assert text in ints
    assert ints[b"-2147483649"] is None and ints[b"4294967296"] is None and ints[b"12345678901"] is None and ints[b"-"] is None and ints[b""] is None
    # the smallest type at every edge
    types = {v: bam.tags_from_comment(b"@r\tXI:i:%d" % v, [b"XI"])[0][2:3] for v in ints.values() if v is not None}
    assert types == {-2147483648: b"i", -32769: b"i", -32768: b"s", -129: b"s", -128: b"c", -1: b"c", 0: b"C", 255: b"C", 256: b"S", 65535: b"S",
                     65536: b"I", 4294967295: b"I", 5: b"C", 7: b"C"}


def test_from_fastq_appends_the_tags_and_counts_them():
    text = b"".join(b"@r%d%s\nACGT\n+\nIIII\n" % (k, c[1][3:].split(b"\n")[0].replace(b"\r", b"")) for k, c in enumerate(UT.CASES) if c[1].startswith(b"@r1"))
    names = [b"XI", b"RG", b"MM", b"ML"]
    plain, tagged = bam.from_fastq(text), bam.from_fastq(text, tags=names)
    assert bam.from_fastq(text, tags=None) == bam.from_fastq(text, tags=[]) == plain
    a, b = list(bam.records(HEADER + plain)), list(bam.records(HEADER + tagged))
    heads = text.split(b"\n")[0::4]
    want = dict.fromkeys(("malformed_records", "float_values_skipped"), 0)
    copied = [0] * len(names)
    for x, y, head in zip(a, b, heads):
        tags, c, mal, fl = bam.tags_from_comment(head, names)
        bx, by = (HEADER + plain)[x.offset:x.offset + x.size], (HEADER + tagged)[y.offset:y.offset + y.size]
        assert by[4:] == bx[4:] + tags and struct.unpack_from("<i", by)[0] == struct.unpack_from("<i", bx)[0] + len(tags)      # block_size includes them
        want["malformed_records"] += mal
        want["float_values_skipped"] += fl
        copied = [p + q for p, q in zip(copied, c)]
    got = bam.ubam_tag_counts(text, names)
    assert got == dict(want, copied=copied) and got["malformed_records"] > 10 and got["float_values_skipped"] > 0 and min(copied[:2]) > 0


def _originals():
    """BAM data of the well-formed records of tests/bam_tags_cases.py and of random ones; the names hold no white space"""
    recs = [r for _, r, want in BT.CASES if want != "malformed" and not _.startswith("decoy")] + BT.random_records(5, 300, damaged_every=10 ** 9)
    return HEADER + b"".join(recs)


@pytest.mark.parametrize("names", [[b"RG"], [b"ML", b"RG", b"NM", b"MM"],
                                   [b"RG", b"XA", b"XC", b"Xc", b"XS", b"Xs", b"XI", b"Xi", b"Xf", b"XZ", b"XH", b"BC", b"NM", b"ML", b"AB", b"ZZ"]],
                         ids=["RG", "four", "sixteen"])
def test_text_fixed_point(names):
    d = _originals()
    t = bam.fastq_text_tagged(d, names)
    assert t.count(b"\t") > 100
    back = HEADER + bam.from_fastq(t, tags=names)
    assert bam.fastq_text_tagged(back, names) == t
    # the binary tags are the originals', scalar integers in the smallest type
    n_checked = 0
    for x, y in zip(bam.records(d), bam.records(back)):
        if bam.tag_comment(d, x.offset, names)[2]:
            assert bam.find_tag(back, y.offset, names[0])[0] == bam.TAG_NONE
            continue
        for name in names:
            off, n, ty = bam.find_tag(d, x.offset, name)
            off2, n2, ty2 = bam.find_tag(back, y.offset, name)
            if off == bam.TAG_NONE or ty == ord("f") or (ty == ord("B") and d[off] == ord("f")):
                assert off2 == bam.TAG_NONE
            elif ty in bam._TAG_INT:
                v = struct.unpack(bam._TAG_INT[ty], d[off:off + n])[0]
                assert struct.unpack(bam._TAG_INT[ty2], back[off2:off2 + n2])[0] == v and bytes([ty2]) == bam._small_int(v)[0]
            else:
                assert (ty2, back[off2:off2 + n2]) == (ty, d[off:off + n])
            n_checked += 1
    assert n_checked > 300


def test_a_tag_takes_at_most_twice_its_text():
    rnd = random.Random(11)
    names = [b"MM", b"ML", b"RG", b"XI"]
    grew = 0
    for _ in range(3000):
        f = UT.random_field(rnd)
        tags = bam.tags_from_comment(b"@r\t" + f, names)[0]
        assert len(tags) <= max(len(f), 2 * len(f) - 4), f
        grew += len(tags) > len(f)
    assert grew > 0, "a B array of small i / I values grows"
    assert len(bam.tags_from_comment(b"@r\tXI:B:I,1,2,3", names)[0]) == 2 * len(b"XI:B:I,1,2,3") - 4
    # whole records: the tags within 2 x the comment, the raw bytes within the bound of the untagged records plus what the tags exceed the comment by
    text, over, n = [], 0, 2000
    for k in range(n):
        comment = b"\t".join(UT.random_field(rnd) for _ in range(rnd.randrange(0, 5)))
        head = b"@r%d" % k + (rnd.choice((b" ", b"\t")) + comment if rnd.random() < 0.9 else b"")
        tags = bam.tags_from_comment(head, names)[0]
        c = bam.ubam_comment(head)
        assert len(tags) <= 2 * len(c or b"")
        over += max(0, len(tags) - len(c) - 1) if c is not None else 0
        ls = rnd.randrange(0, 30)
        text.append(head + b"\n" + b"A" * ls + b"\n+\n" + b"I" * ls + b"\n")
    text = b"".join(text)
    assert len(bam.from_fastq(text, tags=names)) <= bam.ubam_bound(len(text), n) + over


def test_the_rules_of_the_flag(monkeypatch):
    from ribodetector_amd import detect
    monkeypatch.delenv("RD_DEVICE_PARSE", raising=False)
    monkeypatch.delenv("RD_INGEST", raising=False)
    on_device = lambda p: True      # noqa: E731
    assert detect.check_ubam(True, ["a.fq"], ["o.bam"], ["r.bam"], parse_wanted=on_device, ubam_tags="MM,ML,RG") == [b"MM", b"ML", b"RG"]
    assert detect.check_ubam(True, ["a.fq"], ["o.bam"], ["r.bam"], parse_wanted=on_device) is None
    assert detect.check_ubam_tags(None, False) is None
    with pytest.raises(RuntimeError, match="--ubam_tags .* give --ubam_output with it"):
        detect.check_ubam(False, ["a.fq"], ["o.fq"], None, ubam_tags="MM")
    for bad, why in (("", "empty"), ("M", "not a tag name"), ("MM,1M", "not a tag name"), ("MM,MM", "twice"),
                     (",".join("X%c" % (65 + j) for j in range(17)), "more than 16")):
        with pytest.raises(RuntimeError, match="--ubam_tags: .*" + why):
            detect.check_ubam(True, ["a.fq"], ["o.bam"], None, parse_wanted=on_device, ubam_tags=bad)
    parser = detect.build_parser()
    assert parser.parse_args(["-l", "100", "-i", "a.fq", "-o", "o.bam", "--ubam_output", "--ubam_tags", "MM,ML"]).ubam_tags == "MM,ML"
    assert parser.parse_args(["-l", "100", "-i", "a.fq", "-o", "o.fq"]).ubam_tags is None


def test_the_summary_object_and_the_log_line():
    from ribodetector_amd import ubam
    names = [b"MM", b"RG"]
    one = {"copied": [3, 5], "malformed_records": 1, "float_values_skipped": 2}
    two = {"copied": [4, 0], "malformed_records": 0, "float_values_skipped": 7}
    assert ubam.to_json_tags(names, [one]) == {"tags": ["MM", "RG"], "copied": [3, 5], "malformed_records": 1, "float_values_skipped": 2}
    doc = ubam.to_json_tags(names, [one, two])
    assert doc == {"tags": ["MM", "RG"], "copied": [[3, 4], [5, 0]], "malformed_records": [1, 0], "float_values_skipped": [2, 7]}
    assert list(doc) == ["tags", "copied", "malformed_records", "float_values_skipped"]
    assert ubam.log_line_tags(names, [one, two]) == "BAM tags from text: MM 7, RG 5 copied; 1 records with malformed tags, 9 float values skipped"
