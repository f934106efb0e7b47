"""--split_groups on the GPU: every output file of a run as a family of files, one per read group of mate 1's BAM header and one for
the rest, against the plain statement tests/group_truth.py and against the unsplit run of the same arguments."""
import gzip
import json
import logging
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_truth as GT  # noqa: E402
import test_gpu_bam as G  # noqa: E402
import test_interleaved_host as H  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [b"lib7", b"a/b %", b"empty"]                     # header order; 'empty' has no reads; one id holds '/', a space and '%'
SORTED = bam.sorted_ids(IDS)[0]
HEADER = b"@HD\tVN:1.6\n" + b"".join(b"@RG\tID:" + i + b"\tSM:s\n" for i in IDS)
LABEL = {b"rRNA": 1, b"nonrRNA": 0, b"unclassified": -1}
SMALL = ["--chunk_size", "1", "-m", "3"]                # 1,024 reads / 512 pairs per chunk: four chunks of the files below


def _tagged(reads, rng, shift=0):
    """the reads with an RG of every kind (declared, none, undeclared, RG:i, cut short) and secondary records in between"""
    out = []
    for i, r in enumerate(reads):
        kind = (int(rng.integers(0, 9)) + shift) % 9
        tags = b"NMi" + struct.pack("<i", i % 7) + b"xff" + struct.pack("<f", 0.25 * i)
        if kind < 4:
            tags += b"RGZ" + IDS[kind % 2] + b"\0"
        elif kind == 4:
            tags += b"RGZnobody\0"
        elif kind == 5:
            tags += b"RGi" + struct.pack("<i", 5)
        elif kind == 6:
            tags += b"RGZcut"
        out.append(dict(r, tags=tags))
        if i % 97 == 5:
            out.append(dict(r, name=r["name"] + b".sec", flag=r.get("flag", 4) | 0x100, tags=b"RGZlib7\0"))
    return out


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("splitsets")
    rng = np.random.default_rng(77)
    a, o, _ = synth.reads_numpy(3300, (60, 120), seed=41, rrna_frac=0.3)
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(1700, (60, 120), seed=32, rrna_frac=0.3), synth.reads_numpy(1700, (60, 120), seed=33, rrna_frac=0.3)
    r1, r2 = G._bam_reads(a1, o1, mate=1, rng=rng), G._bam_reads(a2, o2, mate=2, rng=rng)
    t1, t2 = _tagged(r1, rng), [dict(r, tags=b"RGZempty\0") for r in r2]      # (mate 2's own RG is not consulted)
    il = _tagged(H.interleave(r1, r2), rng)
    out = {}
    for name, reads in (("se", _tagged(G._bam_reads(a, o, rng=rng), rng)), ("m1", t1), ("m2", t2), ("il", il)):
        path = str(d / (name + ".bam"))
        out[name] = (path, bam.write_bam(path, reads, text=HEADER))
    return out


LAYOUTS = {"se": (["se"], 1, False), "pe": (["m1", "m2"], 2, False), "il1": (["il"], 1, True), "il2": (["il"], 2, True)}


def _run(tmp_path, sets, layout, ensure, exts, extra=(), split=True, tag=""):
    """one run; returns (the Predictor, the output paths [-o..., -r...], the directory)"""
    names, outs, inter = LAYOUTS[layout]
    d = tmp_path / ("%s_%s_%s%s" % (layout, ensure, "split" if split else "whole", tag))
    d.mkdir()
    o, r = [str(d / ("o%d%s" % (k, exts[0]))) for k in range(outs)], [str(d / ("r%d%s" % (k, exts[1]))) for k in range(outs)]
    args = ["-l", "100", "-e", ensure, "-i", *[sets[n][0] for n in names], "-o", *o, "-r", *r, "--read_report", str(d / "rep.tsv")]
    p = G._run(args + (["--interleaved"] if inter else []) + (["--split_groups"] if split else []) + list(extra) + SMALL)
    return p, o + r, d


def _read(path):
    """the bytes of an output file, inflated where its name says it is compressed (.gz, and BGZF under .bam / .ubam)"""
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if path.endswith(("gz", ".bam", ".ubam")) else raw


def _labels(d):
    lines = open(str(d / "rep.tsv"), "rb").read().split(b"\n")[1:-1]
    return [LABEL[x.split(b"\t")[1]] for x in lines]


def _ids_of(text):
    return [x.split(b"\t")[0].split(b" ")[0] for x in text.split(b"\n")[0::4] if x]


def _check_families(sets, layout, ensure, exts, whole, split, source="fastq", tags=None, floats=False):
    """the files of the split run against the statement and against the unsplit run's files"""
    (pw, wpaths, wd), (ps, spaths, sd) = whole, split
    names, outs, inter = LAYOUTS[layout]
    labels = _labels(wd)
    assert labels == _labels(sd) and open(str(wd / "rep.tsv"), "rb").read() == open(str(sd / "rep.tsv"), "rb").read()
    paired = layout != "se"
    fams = [(0, wpaths[:outs], spaths[:outs]), (1, wpaths[outs:], spaths[outs:])]
    if paired and ensure == "both":
        unc = ".unclassified.bam" if source == "raw" else ".unclassified.gz"
        fams.append((-1, [x + unc for x in wpaths[:outs]], [x + unc for x in spaths[:outs]]))
    want_files = {os.path.basename(m) for _, _, sp in fams for x in sp for m in bam.split_paths(x, SORTED)} | {"rep.tsv"}
    assert set(os.listdir(str(sd))) == want_files
    rows1 = GT.group_rows(sets[names[0]][1], IDS)
    for label, wp, sp in fams:
        per_mate = []
        for e in range(outs):
            data = sets[names[e if not inter else 0]][1]
            if inter:
                fam = GT.split_select(data, labels, IDS, label, source, tags, floats, 0, 2, None if outs == 1 else e)
            else:
                fam = GT.split_select(data, labels, IDS, label, source, tags, floats, rows=rows1)
            got = []
            for g, m in enumerate(bam.split_paths(sp[e], SORTED)):
                body = _read(m)
                if source == "raw":
                    assert body[:bam.header_len(body)] == data[:bam.header_len(data)], m
                    body = body[bam.header_len(body):]
                assert body == fam[g], (m, len(body), len(fam[g]))
                got.append(body)
            if source != "raw":
                empty = str(sd / ("empty_probe" + os.path.splitext(sp[e])[1]))
                from ribodetector_amd.data_loader import fastx_parser as fx
                fx.open_for_write(empty).close()
                assert open(bam.split_name(sp[e], b"empty"), "rb").read() == open(empty, "rb").read() and got[SORTED.index(b"empty")] == b""
                os.remove(empty)
            unsplit = _read(wp[e])
            if source == "raw":
                unsplit = unsplit[bam.header_len(unsplit):]
            assert sum(len(b) for b in got) == len(unsplit)
            # merged in input order: walk the unsplit file, every record must be the next bytes of exactly its member
            if source != "raw":
                cur = [0] * len(got)
                units = [k for k, lab in enumerate(labels) if lab == label]
                at = 0
                for k in units:
                    g = min(rows1[k * (2 if inter else 1)], len(IDS))
                    lines = 4 * (2 if inter and outs == 1 else 1)
                    end = cur[g]
                    for _ in range(lines):
                        end = got[g].index(b"\n", end) + 1
                    assert unsplit[at:at + end - cur[g]] == got[g][cur[g]:end], (label, e, k)
                    at, cur[g] = at + end - cur[g], end
                assert at == len(unsplit) and cur == [len(b) for b in got]
            per_mate.append(got)
        if outs == 2 and source != "raw":                   # the mate files of a group hold the same ids in the same order
            for g in range(len(SORTED) + 1):
                a, b = _ids_of(per_mate[0][g]), _ids_of(per_mate[1][g])
                assert [x.rsplit(b"/", 1)[0] for x in a] == [x.rsplit(b"/", 1)[0] for x in b]


CASES = [("se", "rrna", (".fq", ".fq.gz")), ("se", "rrna", (".fq.gz", ".fq.gz")), ("se", "rrna", (".fq", ".fq"))] + \
        [(lay, ens, (".fq", ".fq.gz") if k % 2 else (".fq.gz", ".fq")) for lay in ("pe", "il1", "il2")
         for k, ens in enumerate(("rrna", "norrna", "both", "none"))]


@pytest.mark.parametrize("layout,ensure,exts", CASES)
def test_families_against_the_statement_and_the_unsplit_run(tmp_path, sets, layout, ensure, exts):
    whole = _run(tmp_path, sets, layout, ensure, exts, split=False)
    split = _run(tmp_path, sets, layout, ensure, exts)
    assert whole[0].num_read >= 1700 and (whole[0].num_read, whole[0].num_rrna) == (split[0].num_read, split[0].num_rrna)
    _check_families(sets, layout, ensure, exts, whole, split)


def test_bam_output_members_keep_the_header_and_the_records(tmp_path, sets):
    whole = _run(tmp_path, sets, "pe", "both", (".bam", ".ubam"), extra=["--bam_output"], split=False)
    split = _run(tmp_path, sets, "pe", "both", (".bam", ".ubam"), extra=["--bam_output"])
    _check_families(sets, "pe", "both", (".bam", ".ubam"), whole, split, source="raw")
    for m in bam.split_paths(split[1][0], SORTED):
        body = _read(m)
        assert all(not r.skipped for r in bam.records(body))


def test_tagged_members(tmp_path, sets):
    extra = ["--bam_tags", "RG,NM,xf", "--bam_tag_floats"]
    whole = _run(tmp_path, sets, "se", "rrna", (".fq", ".fq.gz"), extra=extra, split=False)
    split = _run(tmp_path, sets, "se", "rrna", (".fq", ".fq.gz"), extra=extra)
    _check_families(sets, "se", "rrna", (".fq", ".fq.gz"), whole, split, source="tagged", tags=[b"RG", b"NM", b"xf"], floats=True)


def test_summary_counters_and_log(tmp_path, sets, caplog):
    out = []
    for split in (False, True):
        d = tmp_path / ("sum%d" % split)
        d.mkdir()
        args = ["-l", "100", "-e", "both", "-i", sets["m1"][0], sets["m2"][0], "-o", str(d / "o0.fq"), str(d / "o1.fq"), "-r", str(d / "r0.fq.gz"),
                str(d / "r1.fq.gz"), "--summary", str(d / "s.json"), "--read_groups"] + (["--split_groups"] if split else []) + SMALL
        caplog.clear()
        with caplog.at_level(logging.INFO):
            p = G._run(args)
        out.append((p, json.load(open(str(d / "s.json"))), caplog.text))
    (pw, dw, _), (ps, ds, log) = out
    assert list(ds)[-1] == "split_groups" and "split_groups" not in dw
    assert json.dumps(ds["read_groups"]) == json.dumps(dw["read_groups"])
    rg = ds["read_groups"]
    un = {c: sum(rg[k]["units"][c] for k in ("none", "undeclared", "malformed_tags")) for c in ("unclassified", "nonrRNA", "rRNA")}
    assert ds["split_groups"] == {"groups": 3, "files": 24, "unassigned": un}
    assert "Split outputs: 3 read groups + unassigned, 24 files; %d reads unassigned" % sum(un.values()) in log


def test_nothing_changes_without_the_flag(tmp_path, sets):
    """two runs of the same command without --split_groups, one with an unrelated variable in the environment: the same bytes"""
    res = []
    for k, env in enumerate((None, {"RD_UNRELATED": "1"})):
        d = tmp_path / ("plain%d" % k)
        d.mkdir()
        args = ["-l", "100", "-e", "rrna", "-i", sets["se"][0], "-o", str(d / "o.fq.gz"), "-r", str(d / "r.fq"), "--summary", str(d / "s.json")] + SMALL
        G._run(args, env)
        doc = json.load(open(str(d / "s.json")))
        res.append((G._read(str(d / "o.fq.gz")), G._read(str(d / "r.fq")), sorted(os.listdir(str(d))), json.dumps(doc).replace(str(d), "")))
    assert res[0] == res[1] and "split_groups" not in res[0][3]
