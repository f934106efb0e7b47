"""The tag walk, the @RG dictionary and the row rule in plain Python (bam.find_tag / read_groups / group_row), the argument rules of
--read_groups, and groups.to_json on a hand-made accumulator. No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402


# ---- find_tag -------------------------------------------------------------------------------------------------------------------------
def test_find_tag_on_the_hand_built_cases():
    """every case says what its construction says - alone, and inside a view where the next record's bytes follow at once"""
    recs = [c[1] for c in T.CASES]
    raw, st = T.view(recs)
    for k, (name, r, want) in enumerate(T.CASES):
        alone = bam.find_tag(r, 0, T.TARGET)
        assert T.check_case(r, 0, len(r), alone, want), (name, alone, want)
        in_view = bam.find_tag(raw, st[k], T.TARGET)       # (the whole view behind it: the record's own end must stop the walk)
        assert T.check_case(raw, st[k], st[k + 1], in_view, want), (name, in_view, want)
        assert in_view == ((alone[0] + st[k],) + alone[1:] if alone[0] >= 0 else alone), name
    assert T.reference(raw, st) == [bam.find_tag(raw, st[k], T.TARGET) for k in range(len(recs))]
    kinds = [c[2] if isinstance(c[2], str) else "found" for c in T.CASES]
    assert min(kinds.count(k) for k in ("found", "none", "malformed")) >= 8


def test_find_tag_values_and_offsets():
    tags = T.scalar(b"NM", "i", 5) + T.Z(b"RG", b"ab") + T.B(b"ML", "S", [1, 2, 3]) + T.Z(b"XH", b"0F", "H")
    r = T.rec(tags, name=b"q", seq="ACG")
    t0 = 36 + 2 + 2 + 3
    assert bam.find_tag(r, 0, b"NM") == (t0 + 3, 4, ord("i"))
    assert bam.find_tag(r, 0, b"RG") == (t0 + 7 + 3, 2, ord("Z"))
    assert bam.find_tag(r, 0, b"ML") == (t0 + 7 + 6 + 3, 5 + 6, ord("B"))
    assert bam.find_tag(r, 0, b"XH") == (t0 + 7 + 6 + 14 + 3, 2, ord("H"))
    assert bam.find_tag(r, 0, b"ZZ") == (-1, 0, 0)
    assert bam.find_tag(b"\0" * 10 + r, 10, b"RG") == (10 + t0 + 10, 2, ord("Z"))
    # a record that does not lie inside the data, a block_size that cannot hold the fixed part
    assert bam.find_tag(r[:-1], 0, b"RG") == (-2, 0, 0) and bam.find_tag(r, 1 << 20, b"RG") == (-2, 0, 0)
    assert bam.find_tag(struct.pack("<i", 31) + r[4:], 0, b"RG") == (-2, 0, 0)
    with pytest.raises(ValueError):
        bam.find_tag(r, 0, b"RGX")


def test_find_tag_random_lists_never_leave_the_record():
    """the seeded sweep the GPU test runs too: a result is none, malformed, or a value inside the record's own tags"""
    recs = T.random_records(7, 300)
    raw, st = T.view(recs)
    ref = T.reference(raw, st)
    assert ref == [bam.find_tag(raw, st[k], T.TARGET) for k in range(300)]
    seen = {"found": 0, "none": 0, "malformed": 0}
    for k, (off, ln, t) in enumerate(ref):
        if off >= 0:
            assert st[k] + 36 <= off - 3 and off + ln <= st[k + 1] and raw[off - 3:off - 1] == T.TARGET and raw[off - 1] == t
        else:
            assert (ln, t) == (0, 0) and off in (-1, -2)
        seen["found" if off >= 0 else "none" if off == -1 else "malformed"] += 1
    assert min(seen.values()) >= 15, seen


# ---- read_groups, group_row -----------------------------------------------------------------------------------------------------------
def _header(text):
    return bam.encode_header(refs=[(b"chr1", 100)], text=text)


def test_read_groups():
    text = (b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:lib2\tSM:s2\tBC:ACGT-TTGA\tLB:L\tPL:ONT\tDS:a b:c\n@CO\t@RG\tID:not\n"
            b"@RG\tSM:first\tID:lib1\n@RG\tID:\xe9\n@PG\tID:lib1\n")
    got = bam.read_groups(_header(text))
    assert [g[0] for g in got] == [b"lib2", b"lib1", b"\xe9"]
    assert got[0][1] == {"ID": "lib2", "SM": "s2", "BC": "ACGT-TTGA", "LB": "L", "PL": "ONT", "DS": "a b:c"}
    assert got[1][1] == {"SM": "first", "ID": "lib1"} and got[2][1] == {"ID": "\xe9"}
    assert bam.read_groups(_header(b"")) == [] and bam.read_groups(_header(b"@HD\tVN:1.6\n")) == []
    assert bam.read_groups(_header(b"@RG\tID:a\n\0\0\0")) == [(b"a", {"ID": "a"})]          # (NUL padding behind the text)
    for bad, word in ((b"@RG\tSM:x\n", "without ID"), (b"@RG\tID:\tSM:x\n", "empty ID"), (b"@RG\tID:a\n@RG\tID:b\n@RG\tID:a\tSM:y\n", "duplicate @RG ID 'a'")):
        with pytest.raises(ValueError, match=word):
            bam.read_groups(_header(bad))
    with pytest.raises(ValueError):
        bam.read_groups(b"@RG\tID:a\n")


def test_sorted_ids_and_group_row():
    ids = [b"b", b"abc", b"\xe9x", b"a", b"ab", b"Z"]
    srt, order = bam.sorted_ids(ids)
    assert srt == [b"Z", b"a", b"ab", b"abc", b"b", b"\xe9x"] and [ids[j] for j in order] == srt        # unsigned bytes: 0xe9 last
    G = len(ids)

    def row(tags, names=ids):
        r = T.rec(tags)
        return bam.group_row(r, *bam.find_tag(r, 0, b"RG"), names)
    for j, rid in enumerate(ids):
        assert row(T.scalar(b"NM", "i", 1) + T.Z(b"RG", rid)) == j
    assert row(b"") == G and row(T.scalar(b"NM", "i", 1)) == G
    for other in (b"", b"abcd", b"A", b"\xe9", b"\xe9xx", b"c"):
        assert row(T.Z(b"RG", other)) == G + 1
    assert row(T.scalar(b"RG", "i", 5)) == G + 2 and row(T.Z(b"RG", b"a", "H")) == G + 2       # not of type Z
    assert row(b"RGZa") == G + 2 and row(T.scalar(b"NM", "i", 1) + b"RG") == G + 2             # malformed
    assert row(b"", names=[]) == 0 and row(T.Z(b"RG", b"a"), names=[]) == 1 and row(b"RG", names=[]) == 2


# ---- the argument rules ---------------------------------------------------------------------------------------------------------------
def _bam(tmp_path, name, text):
    path = str(tmp_path / name)
    bam.write_bam(path, [dict(name=b"r", seq="ACGT", qual=bytes(4), tags=T.Z(b"RG", b"a"))], text=text)
    return path


def test_argument_rules_hold_before_a_device_is_touched(tmp_path, monkeypatch):
    """each one is a RuntimeError of detect.main; the model is never loaded (Predictor.load_model would be the first device call)"""
    from ribodetector_amd import detect
    monkeypatch.setattr(detect.Predictor, "load_model", lambda self: pytest.fail("the run went on to load the model"))
    good = _bam(tmp_path, "good.bam", b"@RG\tID:a\tSM:s\n@RG\tID:b\n")
    out = ["-o", str(tmp_path / "o.fq"), "-l", "100"]
    js = ["--summary", str(tmp_path / "s.json")]
    with pytest.raises(RuntimeError, match="--summary PATH"):
        detect.main(["-i", good, "--read_groups"] + out)
    fq = str(tmp_path / "x.fq")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    with pytest.raises(RuntimeError, match="must end with .bam or .ubam"):
        detect.main(["-i", fq, "--read_groups"] + js + out)
    with pytest.raises(RuntimeError, match="duplicate @RG ID 'a'.*before anything touches a device"):
        detect.main(["-i", _bam(tmp_path, "dup.bam", b"@RG\tID:a\n@RG\tID:a\n"), "--read_groups"] + js + out)
    with pytest.raises(RuntimeError, match="empty ID"):
        detect.main(["-i", _bam(tmp_path, "empty.bam", b"@RG\tID:\tSM:x\n"), "--read_groups"] + js + out)
    with pytest.raises(RuntimeError, match="without ID"):
        detect.main(["-i", _bam(tmp_path, "noid.bam", b"@RG\tSM:x\n"), "--read_groups"] + js + out)
    many = b"".join(b"@RG\tID:g%d\n" % k for k in range(65537))
    with pytest.raises(RuntimeError, match="65537 read groups, more than 65536"):
        detect.main(["-i", _bam(tmp_path, "many.bam", many), "--read_groups"] + js + out)
    with pytest.raises(RuntimeError, match="cannot read the header"):
        detect.main(["-i", str(tmp_path / "missing.bam"), "--read_groups"] + js + out)
    # the checks themselves: nothing without the flag, the declared groups with it
    assert detect.check_read_groups(False, None, [fq]) is None
    assert [g[0] for g in detect.check_read_groups(True, js[1], [good])] == [b"a", b"b"]
    assert len(detect.check_read_groups(True, js[1], [_bam(tmp_path, "max.bam", many[:many.rindex(b"@RG")])])) == 65536
    assert detect.build_parser().parse_args(["-i", good, "-o", "o.fq", "-l", "100"]).read_groups is False


# ---- to_json --------------------------------------------------------------------------------------------------------------------------
def test_to_json_maps_sorted_rows_back_to_header_order():
    from ribodetector_amd import groups
    declared = bam.read_groups(_header(b"@RG\tID:zeta\tSM:s1\tBC:AAC\n@RG\tID:alpha\tLB:lib\tPL:PACBIO\n@RG\tID:mid\n"))
    G = 3
    acc = np.zeros(groups.acc_words(G), dtype=np.int64)
    rows = acc[:-1].reshape(G + 3, 3, 2)
    # sorted order: alpha (row 0), mid (row 1), zeta (row 2); then none, undeclared, malformed. [class][units, bases]
    rows[0] = [[1, 100], [2, 250], [7, 1 << 40]]
    rows[2] = [[0, 0], [3, 300], [1, 90]]
    rows[3] = [[0, 0], [1, 10], [0, 0]]
    rows[4] = [[1, 7], [0, 0], [2, 3]]
    rows[5] = [[0, 0], [0, 0], [1, 55]]
    acc[-1] = 4
    doc = groups.to_json(acc, declared, True, input="in.bam")
    assert list(doc) == ["tag", "input", "groups", "none", "undeclared", "malformed_tags", "mate2_differs"]
    assert doc["tag"] == "RG" and doc["input"] == "in.bam" and doc["mate2_differs"] == 4
    assert [g["id"] for g in doc["groups"]] == ["zeta", "alpha", "mid"]
    z, a, m = doc["groups"]
    assert (z["SM"], z["BC"], z["LB"], z["PL"]) == ("s1", "AAC", None, None) and (a["SM"], a["LB"], a["PL"]) == (None, "lib", "PACBIO")
    assert z["units"] == {"total": 4, "nonrRNA": 3, "rRNA": 1, "unclassified": 0, "rRNA_fraction": 0.25}
    assert z["bases"] == {"total": 390, "nonrRNA": 300, "rRNA": 90, "unclassified": 0, "rRNA_fraction": round(90 / 390, 6)}
    assert a["units"] == {"total": 10, "nonrRNA": 2, "rRNA": 7, "unclassified": 1, "rRNA_fraction": 0.7}
    assert a["bases"]["rRNA"] == 1 << 40 and a["bases"]["total"] == (1 << 40) + 350
    assert m["units"] == {"total": 0, "nonrRNA": 0, "rRNA": 0, "unclassified": 0, "rRNA_fraction": None} and m["bases"]["rRNA_fraction"] is None
    assert doc["none"]["units"]["total"] == 1 and doc["undeclared"]["units"] == {"total": 3, "nonrRNA": 0, "rRNA": 2, "unclassified": 1,
                                                                                 "rRNA_fraction": round(2 / 3, 6)}
    assert doc["malformed_tags"]["bases"]["rRNA"] == 55
    assert groups.units_per_class(acc, G) == [2, 6, 11]
    single = groups.to_json(acc, declared, False, input="in.bam")
    assert "mate2_differs" not in single and single["groups"] == doc["groups"]
    none = groups.to_json(np.zeros(groups.acc_words(0), dtype=np.int64), [], False)
    assert none["groups"] == [] and none["none"]["units"]["rRNA_fraction"] is None
    with pytest.raises(ValueError):
        groups.to_json(acc[:-1], declared, True)
    import json
    json.dumps(doc)
