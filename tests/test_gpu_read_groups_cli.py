"""--summary --read_groups on the GPU, through the CLI: the "read_groups" object of the summary is recomputed from the run's own
--read_report (the label of every unit, in input order) and the rule in bam.py (records, find_tag, group_row over the input's inflated
bytes), and compared exactly. Three declared groups (one never used), records without RG, with an undeclared RG, one with malformed
tags, and secondary / supplementary records that carry an RG and are in no count."""
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bam as G  # noqa: E402
import test_interleaved_host as IH  # noqa: E402
import test_read_report_host as H  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

N_READS = 3000
TEXT_1 = b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:lib2\tSM:sample2\tBC:ACGT\tPL:ONT\n@RG\tID:lib1\tSM:sample1\tLB:L1\n@RG\tID:\xe9mpty\tSM:never used\n"
TEXT_2 = b"@HD\tVN:1.6\n@RG\tID:lib1\n@RG\tID:elsewhere\n"             # mate 2's own header: its groups are looked up in mate 1's
CLASSES = ("unclassified", "nonrRNA", "rRNA")
LABELS = {b"unclassified": 0, b"nonrRNA": 1, b"rRNA": 2}


def _tagged(reads, rng, mate2=False, skipped=True):
    out = []
    for i, r in enumerate(reads):
        r = dict(r)
        tags = b"NMi" + struct.pack("<i", i)
        if i % 5 == 0:                                   # a long Z and a B in front of RG
            ml = bytes(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8))
            tags += b"MMZC+m," + b",".join(b"%d" % x for x in rng.integers(0, 9, len(ml))) + b";\0" + b"MLBC" + struct.pack("<I", len(ml)) + ml
        if i % 17 == 3:
            pass                                         # no RG
        elif i % 19 == 5:
            tags += b"RGZghost\0"                        # undeclared
        elif mate2 and i % 23 == 7:
            tags += b"RGZelsewhere\0"                    # declared by mate 2's header only: undeclared for the run
        elif i == 1234 and not mate2:
            tags += b"RGZlib1"                           # no NUL: malformed
        elif mate2 and i % 29 == 11:
            tags += b"RGZlib%d\0" % (1 if i % 10 < 6 else 2)        # (the other group than mate 1's below)
        else:
            tags += b"RGZlib%d\0" % (2 if i % 10 < 6 else 1)
        if i % 7 == 0:
            tags += b"XXZ" + bytes(rng.integers(33, 127, int(rng.integers(0, 40)), dtype=np.uint8)) + b"\0"
        r["tags"] = tags
        out.append(r)
        if skipped and i % 9 == 4:                       # a secondary / supplementary copy with an RG: delivered to nobody, counted nowhere
            out.append(dict(r, flag=r.get("flag", 4) | (0x100 if i % 2 else 0x800), ref_id=0, pos=11, cigar=[(len(r["seq"]), "M")],
                            tags=b"RGZlib1\0"))
    return out


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("read_groups")
    rng = np.random.default_rng(90)
    out = {"dir": d}

    def make(tag, reads, text):
        path = str(d / (tag + ".bam"))
        return path, bam.write_bam(path, reads, text=text, member_bytes=5003)      # (5,003 bytes a member: records straddle the members)
    (a1, o1, _), (a2, o2, _) = (synth.reads_numpy(N_READS, (60, 120), seed=91 + e, rrna_frac=0.4) for e in (0, 1))
    r1 = _tagged(G._bam_reads(a1, o1, mate=1, rng=rng), rng)
    r2 = _tagged(G._bam_reads(a2, o2, mate=2, rng=rng), rng, mate2=True)
    out["a"], out["b"] = make("a", r1, TEXT_1), make("b", r2, TEXT_2)
    keep = lambda rs: [r for r in rs if not r.get("flag", 4) & 0x900]              # noqa: E731  (an interleaved file alternates its DELIVERED records)
    il = IH.interleave(keep(r1), keep(r2))
    il[40:40] = [dict(il[39], flag=0x104, tags=b"RGZlib2\0")]                     # (a skipped record between two pairs)
    out["il"] = make("il", il, TEXT_1)
    return out


def _delivered(data):
    """[(row in header order, l_seq)] of the delivered records of a file, by the rule; the groups are those of mate 1's header"""
    ids = [g[0] for g in bam.read_groups(bam.encode_header(text=TEXT_1))]
    assert ids == [b"lib2", b"lib1", b"\xe9mpty"]
    out = []
    for r in bam.records(data):
        if not r.skipped:
            out.append((bam.group_row(data, *bam.find_tag(data, r.offset, b"RG"), ids), len(r.codes)))
    return out


def _counts(a):
    total = sum(a)
    return {"total": total, "nonrRNA": a[1], "rRNA": a[2], "unclassified": a[0], "rRNA_fraction": round(a[2] / total, 6) if total else None}


def _expected(path, report, mates):
    """the "read_groups" object from the report's labels and the mates' [(row, l_seq)]"""
    _, lines = H.parse(H.read_report(report))
    assert len(lines) == len(mates[0]) and all(len(m) == len(lines) for m in mates)
    G_ = 3
    units, bases = np.zeros((G_ + 3, 3), dtype=np.int64), np.zeros((G_ + 3, 3), dtype=np.int64)
    differs = 0
    for u, ln in enumerate(lines):
        c, g = LABELS[ln[1]], mates[0][u][0]
        units[g, c] += 1
        bases[g, c] += sum(m[u][1] for m in mates)
        differs += len(mates) == 2 and mates[1][u][0] != g
    row = lambda j: {"units": _counts(units[j].tolist()), "bases": _counts(bases[j].tolist())}     # noqa: E731
    hdr = [("lib2", "sample2", "ACGT", None, "ONT"), ("lib1", "sample1", None, "L1", None), ("\xe9mpty", "never used", None, None, None)]
    doc = {"tag": "RG", "input": path,
           "groups": [dict({"id": i, "SM": sm, "BC": bc, "LB": lb, "PL": pl}, **row(j)) for j, (i, sm, bc, lb, pl) in enumerate(hdr)],
           "none": row(3), "undeclared": row(4), "malformed_tags": row(5)}
    if len(mates) == 2:
        doc["mate2_differs"] = int(differs)
    return doc, units


def _run(d, tag, inputs, outs, extra=(), flag=True):
    d = d / tag
    d.mkdir()
    o, r = [str(d / ("o%d.fq" % k)) for k in range(outs)], [str(d / ("r%d.fq.gz" % k)) for k in range(outs)]
    rep, js = str(d / "report.tsv"), str(d / "summary.json")
    p = G._run(["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "--read_report", rep, "--summary", js, *extra] + (["--read_groups"] if flag else []) + G.SMALL)
    files = o + r + [rep] + ([x + ".unclassified.gz" for x in o] if "both" in extra else [])
    assert all(os.path.exists(f) for f in files)
    return p, json.load(open(js)), rep, files


def _check(p, doc, want, units):
    rg = doc["read_groups"]
    assert rg == want
    assert list(rg)[:6] == ["tag", "input", "groups", "none", "undeclared", "malformed_tags"]
    # the rows sum to the run's reads, class by class
    assert [int(x) for x in units.sum(0)] == [doc["reads"][c] for c in CLASSES] == [p.num_unknown, p.num_nonrrna, p.num_rrna]
    rows = rg["groups"] + [rg["none"], rg["undeclared"], rg["malformed_tags"]]
    assert [sum(r["units"][c] for r in rows) for c in CLASSES] == [doc["reads"][c] for c in CLASSES]
    assert rg["groups"][2]["units"]["total"] == 0 and rg["groups"][2]["units"]["rRNA_fraction"] is None            # the group that is never used
    assert min(rg["groups"][k]["units"][c] for k in (0, 1) for c in ("nonrRNA", "rRNA")) > 50
    assert rg["none"]["units"]["total"] > 100 and rg["undeclared"]["units"]["total"] > 100 and rg["malformed_tags"]["units"]["total"] == 1


def test_single_end_and_the_run_without_the_flag(sets):
    path, data = sets["a"]
    recs = list(bam.records(data))
    assert sum(r.skipped for r in recs) > 300 and len(recs) - sum(r.skipped for r in recs) == N_READS
    p, doc, rep, files = _run(sets["dir"], "se", [path], 1)
    assert p.num_read == N_READS and len(p.ingest) == 1
    assert sum(1 for event, _ in p._timeline if event.startswith("chunk_of_")) >= 3          # (chunks of 1,024 reads: the counters add up over them)
    want, units = _expected(path, rep, [_delivered(data)])
    _check(p, doc, want, units)
    assert "mate2_differs" not in doc["read_groups"]
    # the skipped records carry RG:Z:lib1 - counting them would add > 300 units to lib1
    assert doc["read_groups"]["groups"][1]["units"]["total"] == sum(1 for g, _ in _delivered(data) if g == 1)
    # without the flag: no key, and every other output is the same bytes
    p0, doc0, rep0, files0 = _run(sets["dir"], "se_plain", [path], 1, flag=False)
    assert "read_groups" not in doc0
    assert doc0 == {k: v for k, v in doc.items() if k != "read_groups"}
    for f, f0 in zip(files, files0):
        assert open(f, "rb").read() == open(f0, "rb").read(), os.path.basename(f)


def test_two_files(sets):
    (pa, da), (pb, db) = sets["a"], sets["b"]
    p, doc, rep, _ = _run(sets["dir"], "pe", [pa, pb], 2, extra=["-e", "both"])
    assert p.is_paired and p.num_read == N_READS and p.num_unknown > 0
    m1, m2 = _delivered(da), _delivered(db)
    want, units = _expected(pa, rep, [m1, m2])
    _check(p, doc, want, units)
    assert doc["read_groups"]["mate2_differs"] == sum(1 for x, y in zip(m1, m2) if x[0] != y[0]) > 100
    assert sum(1 for x in m2 if x[0] == 4) > sum(1 for x in m1 if x[0] == 4)          # ("elsewhere" is undeclared: mate 1's dictionary)


def test_interleaved(sets):
    path, data = sets["il"]
    p, doc, rep, _ = _run(sets["dir"], "il", [path], 1, extra=["--interleaved", "-e", "both"])
    assert p.is_paired and p.num_read == N_READS
    recs = _delivered(data)
    assert len(recs) == 2 * N_READS
    want, units = _expected(path, rep, [recs[0::2], recs[1::2]])
    _check(p, doc, want, units)
    # the pairs are the two-file run's pairs: the same object up to the input's name
    want_pe, _ = _expected(path, rep, [_delivered(sets["a"][1]), _delivered(sets["b"][1])])
    assert want_pe == want
