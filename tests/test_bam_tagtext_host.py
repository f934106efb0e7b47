"""BAM tags in the FASTQ header lines, the rule (bam.tag_comment, bam.fastq_text_tagged, bam.parse_tag_list) and the refusals of
--bam_tags: pure host code. The comments are compared with byte strings written by hand (tests/bam_tagtext_cases.py), not with the rule
itself."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tagtext_cases as TC  # noqa: E402
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RD_BGZF_SHARD")


def _comment(tags, lst, **kw):
    r = TC.rec(tags, **kw)
    data = TC.file_data([r])
    return bam.tag_comment(data, bam.header_len(data), lst)


@pytest.mark.parametrize("k", range(len(TC.CASES)), ids=[c[0].replace(" ", "_") for c in TC.CASES])
def test_tag_comment_against_literals(k):
    name, tags, lst, want = TC.CASES[k]
    comment, copied, malformed, floats = _comment(tags, lst)
    if want == TC.MALFORMED:
        assert (comment, copied, malformed, floats) == (b"", [False] * len(lst), True, 0)
    else:
        assert comment == want and not malformed and floats == TC.FLOATS.get(name, 0)
        assert sum(copied) == want.count(b"\t") and len(copied) == len(lst)
    assert b"\n" not in comment and all(c == 9 or 0x20 <= c <= 0x7E for c in comment)


def test_the_cases_cover_what_they_must():
    names = [c[0] for c in TC.CASES]
    for t, v in (("c", -128), ("c", 127), ("C", 255), ("s", -32768), ("S", 65535), ("i", -2147483648), ("I", 4294967295)):
        assert "scalar %s %d" % (t, v) in names
    for t in "cCsSiI":
        assert "scalar %s 0" % t in names and all("B:%s of %d" % (t, n) in names for n in (0, 1, 3))


def test_copied_says_which_tags():
    tags = T.Z(b"RG", b"g") + T.scalar(b"qs", "f", 1.0) + T.scalar(b"NM", "i", 3)
    assert _comment(tags, [b"NM", b"MM", b"qs", b"RG"]) == (b"\tNM:i:3\tRG:Z:g", [True, False, False, True], False, 1)


def test_reverse_strand_and_skipped_records():
    tags = T.Z(b"MM", b"C+m,1;") + T.B(b"ML", "C", [200, 3])
    recs = [TC.rec(tags, name=b"fwd", seq="AACCG", flag=4), TC.rec(tags, name=b"rev", seq="AACCG", flag=0x14),
            TC.rec(tags, name=b"sec", seq="AACCG", flag=0x104), TC.rec(tags, name=b"sup", seq="AACCG", flag=0x804), TC.rec(b"", name=b"bare", seq="AC")]
    data = TC.file_data(recs)
    got = bam.fastq_text_tagged(data, [b"ML", b"MM"])
    c = b"\tML:B:C,200,3\tMM:Z:C+m,1;"
    assert got == b"@fwd" + c + b"\nAACCG\n+\n!!!!!\n" + b"@rev" + c + b"\nCGGTT\n+\n!!!!!\n" + b"@bare\nAC\n+\n!!\n"
    assert bam.tag_counts(data, [b"ML", b"MM"]) == {"copied": [2, 2], "malformed_records": 0, "float_values_skipped": 0}


def test_equals_fastq_text_when_no_listed_tag_is_present():
    recs, _ = TC.random_records(3, 200, malformed=0.0)
    data = TC.file_data(recs)
    assert bam.fastq_text_tagged(data, [b"ZZ", b"Y1"]) == bam.fastq_text(data)
    assert bam.tag_counts(data, [b"ZZ", b"Y1"]) == {"copied": [0, 0], "malformed_records": 0, "float_values_skipped": 0}
    body = data[bam.header_len(data):]
    assert bam.fastq_text_tagged(body, [b"ZZ"], start=0) == bam.fastq_text(data)


def test_the_tagged_text_parses_as_the_same_fastq(tmp_path):
    """the project's own host parser reads the tagged text: the same ids (a header line's first word), sequences and qualities"""
    from ribodetector_amd.data_loader import fastx_parser as fx
    recs, lst = TC.random_records(4, 400)
    data = TC.file_data(recs)
    tagged, plain = bam.fastq_text_tagged(data, lst), bam.fastq_text(data)
    assert len(tagged) > len(plain) + 1000
    seen = []
    for text, name in ((plain, "plain.fq"), (tagged, "tagged.fq")):
        path = str(tmp_path / name)
        open(path, "wb").write(text)
        rows = []
        for c in fx.get_seq_chunks(path, chunk_size=150):
            buf = bytes(c.buf)
            for i in range(len(c.seq_len)):
                a, b = int(c.rec_start[i]), int(c.rec_start[i + 1])
                lines = buf[a:b].split(b"\n")
                rows.append((fx.record_id(c.buf, a, b), buf[int(c.seq_off[i]):int(c.seq_off[i]) + int(c.seq_len[i])], lines[3]))
                assert lines[1] == rows[-1][1]
        seen.append(rows)
    assert seen[0] == seen[1] and len(seen[0]) == 400
    assert [r[0] for r in seen[0]] == [b"read%d" % k for k in range(400)]


@pytest.mark.parametrize("text, msg", [("", "empty"), ("M", "not a tag name"), ("MMM", "not a tag name"), ("1M", "not a tag name"), ("M_", "not a tag name"),
                                       ("MM,,ML", "not a tag name"), ("MM, ML", "not a tag name"), ("MM,ML,MM", "appears twice"),
                                       (",".join("A" + chr(97 + i) for i in range(17)), "more than 16")])
def test_parse_tag_list_refuses(text, msg):
    with pytest.raises(ValueError, match=msg):
        bam.parse_tag_list(text)


def test_parse_tag_list():
    assert bam.parse_tag_list("MM,ML,RG") == [b"MM", b"ML", b"RG"] and bam.parse_tag_list("x1") == [b"x1"]
    assert len(bam.parse_tag_list(",".join("A" + chr(97 + i) for i in range(16)))) == 16 == bam.TAGS_MAX


@pytest.mark.parametrize("argv, msg", [
    (["-i", "a.fq", "-o", "o.fq", "--bam_tags", "RG"], "every -i file must end with .bam or .ubam"),
    (["-i", "a.fa", "b.fq.gz", "-o", "o1.fq", "o2.fq", "--bam_tags", "RG"], "every -i file must end with .bam or .ubam"),
    (["-i", "a.bam", "-o", "o.bam", "--bam_output", "--bam_tags", "RG"], "give one of the two"),
    (["-i", "a.bam", "-o", "o.fq", "--bam_tags", ""], "the tag list is empty"),
    (["-i", "a.bam", "-o", "o.fq", "--bam_tags", "R"], "not a tag name"),
    (["-i", "a.bam", "-o", "o.fq", "--bam_tags", "RG,RG"], "appears twice"),
    (["-i", "a.bam", "-o", "o.fq", "--bam_tags", ",".join("A" + chr(97 + i) for i in range(17))], "more than 16"),
])
def test_refused_before_anything_touches_a_device(tmp_path, monkeypatch, argv, msg):
    from ribodetector_amd import detect
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(detect.Predictor, "load_model", lambda self: pytest.fail("the model was loaded"))
    argv = ["-l", "100"] + [a if a.startswith("-") or "," in a or len(a) < 3 else str(tmp_path / a) for a in argv]
    with pytest.raises(RuntimeError, match=msg) as e:
        detect.main(argv)
    assert "--bam_tags" in str(e.value) and "before anything touches a device" in str(e.value)


def test_the_flag_is_parsed_and_checked(tmp_path):
    from ribodetector_amd import bamtags, detect
    t = lambda name: str(tmp_path / name)      # noqa: E731
    a = detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.fq", "--bam_tags", "MM,ML"])
    assert a.bam_tags == "MM,ML" and detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.fq"]).bam_tags is None
    assert detect.check_bam_tags(None, [t("a.fq")]) is None
    assert detect.check_bam_tags("MM,ML", [t("a.bam"), t("b.ubam")]) == [b"MM", b"ML"]
    c = [{"copied": [3, 1], "malformed_records": 2, "float_values_skipped": 0}, {"copied": [4, 0], "malformed_records": 0, "float_values_skipped": 5}]
    assert bamtags.log_line([b"MM", b"ML"], c) == "BAM tags: MM 7, ML 1 copied; 2 records with malformed tags, 5 float values skipped"
    assert bamtags.to_json([b"MM", b"ML"], c[:1]) == {"tags": ["MM", "ML"], "copied": [3, 1], "malformed_records": 2, "float_values_skipped": 0}
    assert bamtags.to_json([b"MM", b"ML"], c) == {"tags": ["MM", "ML"], "copied": [[3, 4], [1, 0]], "malformed_records": [2, 0], "float_values_skipped": [0, 5]}
    assert bamtags.from_vector(bamtags.as_vector(c, 2), 2, 2) == c
    assert bamtags.default_hint(1000, 700) == 2400
