"""BAM tags in the FASTQ header lines on the GPU (C ABI rd_bam_tag_splice, csrc/rd_bam_tagtext.hpp; the CLI's --bam_tags) against the
rule in bam.py (tag_comment, fastq_text_tagged). The views are records of bam.encode_record: their FASTQ text next to the records as
they stand, back to back; both lane mappings of the kernels (RD_TAG_LANES) see the kernel-level cases."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tagtext_cases as TC  # noqa: E402
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LANES = [None, "4", "16"]


@pytest.fixture
def lanes(monkeypatch):
    def use(v):
        if v is None:
            monkeypatch.delenv("RD_TAG_LANES", raising=False)
        else:
            monkeypatch.setenv("RD_TAG_LANES", v)
    return use


def _views(records):
    """(FASTQ text, rec_start, raw, raw_start) of the records (none of them skipped), as bytes and lists"""
    data = TC.file_data(records)
    recs = list(bam.records(data))
    assert len(recs) == len(records) and not any(r.skipped for r in recs)
    texts = [r.fastq() for r in recs]
    rs = [0]
    for t in texts:
        rs.append(rs[-1] + len(t))
    raw, st = T.view(records)
    return data, b"".join(texts), rs, raw, st


def _want(data, tags):
    """the rule: (tagged text, out_start, counts)"""
    parts = []
    for r in bam.records(data):
        t = r.fastq()
        at = t.index(b"\n")
        parts.append(t[:at] + bam.tag_comment(data, r.offset, tags)[0] + t[at:])
    starts = [0]
    for p in parts:
        starts.append(starts[-1] + len(p))
    text = b"".join(parts)
    assert text == bam.fastq_text_tagged(data, tags)
    return text, starts, bam.tag_counts(data, tags)


def _t(b, pad=b"\xa5" * 64):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) + pad, dtype=np.uint8).copy()).to(DEV)[:len(b)]


def _splice(text, rs, raw, st, tags, cap=None, canary=None):
    import torch
    from ribodetector_amd import bamtags
    n = len(rs) - 1
    d_text, d_raw = _t(text), _t(raw)
    d_rs, d_st = torch.tensor(rs, dtype=torch.int64, device=DEV), torch.tensor(st, dtype=torch.int64, device=DEV)
    cap = len(text) + 5 * len(raw) if cap is None else cap
    out = None
    if canary is not None:
        out = torch.full((((cap + 255) // 256) * 256 + 256,), canary, dtype=torch.uint8, device=DEV)
    out, out_start, info = bamtags.splice(d_text, d_rs, d_raw, d_st, n, tags, cap, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_start.cpu().tolist(), info.cpu().tolist()


def _check(records, tags, exact_cap=False):
    data, text, rs, raw, st = _views(records)
    want, starts, counts = _want(data, tags)
    out, out_start, info = _splice(text, rs, raw, st, tags, cap=len(want) if exact_cap else None)
    assert info[3] == 0 and info[0] == len(records) and info[1] == len(want)
    assert out_start == starts
    got = out[:len(want)].tobytes()
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        r = max(j for j in range(len(starts)) if starts[j] <= k)
        raise AssertionError("record %d differs at byte %d: %r != %r" % (r, k - starts[r], got[starts[r]:starts[r + 1]], want[starts[r]:starts[r + 1]]))
    assert info[4] == counts["malformed_records"] and info[5] == counts["float_values_skipped"]
    assert info[8:8 + len(tags)] == counts["copied"] and not any(info[8 + len(tags):])
    return counts


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", LANES)
def test_splice_on_the_hand_built_cases(lanes, mapping):
    lanes(mapping)
    for k, (name, tags, want_list, want) in enumerate(TC.CASES):
        recs = [TC.case_record(0, T.Z(b"CO", b"before")), TC.case_record(k, tags, flag=0x10 if k % 3 == 0 else 4), TC.case_record(2, b"")]
        data, text, rs, raw, st = _views(recs)
        out, out_start, info = _splice(text, rs, raw, st, want_list)
        comment = b"" if want == TC.MALFORMED else want
        r = list(bam.records(data))[1].fastq()
        at = r.index(b"\n")
        assert out[out_start[1]:out_start[2]].tobytes() == r[:at] + comment + r[at:], name
        assert info[3] == 0 and info[4] == (1 if want == TC.MALFORMED else 0), name
        assert info[5] == TC.FLOATS.get(name, 0), name
    # and all of them in one view, against the rule
    for lst in ([b"RG"], [b"ML", b"RG", b"NM", b"XX", b"XA", b"XH", b"MM", b"CO", b"qs", b"XF"]):
        _check([TC.case_record(k, c[1]) for k, c in enumerate(TC.CASES)], lst)


@pytest.mark.parametrize("mapping", LANES)
@pytest.mark.parametrize("n_rec", [1, 63, 64, 65, 257, 2047, 2048, 2049, 3000])      # (2,048 records per workgroup of the scan)
def test_splice_record_counts(lanes, mapping, n_rec):
    lanes(mapping)
    base, lst = TC.random_records(11, 97)
    _check([base[(5 * k + n_rec) % len(base)] for k in range(n_rec)], lst, exact_cap=True)


def test_splice_no_records():
    out, out_start, info = _splice(b"", [0], b"", [0], [b"RG"], cap=16)
    assert out_start == [0] and info == [0] * 24


@pytest.mark.parametrize("mapping", LANES)
def test_splice_every_output_residue(lanes, mapping):
    """comments of 0..40 bytes in consecutive records, twice over: a record's output start takes every residue modulo 16"""
    lanes(mapping)
    recs = []
    for rep in range(2):
        for n in range(41):
            tags = b"" if n == 0 else T.Z(b"CO", b"c" * (n - 6)) if n >= 6 else T.Z(b"XY", b"skip")
            recs.append(T.rec(tags, name=b"n%d_%d" % (rep, n), seq="ACGT" * (3 + n % 5) + "A" * (n % 3)))
    data, text, rs, raw, st = _views(recs)
    _, starts, _ = _want(data, [b"CO"])
    assert set(s % 16 for s in starts) == set(range(16))
    _check(recs, [b"CO"])


@pytest.mark.parametrize("mapping", LANES)
def test_splice_z_and_h_lengths(lanes, mapping):
    lanes(mapping)
    recs = []
    for n in (0, 1, 15, 16, 17, 255, 256, 257, 4097):
        recs.append(T.rec(T.scalar(b"NM", "i", n) + T.Z(b"MM", bytes(33 + (7 * i) % 94 for i in range(n))), name=b"z%d" % n))
        recs.append(T.rec(T.Z(b"XH", bytes(b"0123456789abcdefABCDEF"[(5 * i) % 22] for i in range(n)), "H") + T.Z(b"RG", b"g"), name=b"h%d" % n))
        if n:
            bad = bytearray(33 + (7 * i) % 94 for i in range(n))
            bad[n - 1] = 0x0a                              # the last byte of the value is one no header line may hold
            recs.append(T.rec(T.Z(b"MM", bytes(bad)), name=b"b%d" % n))
    c = _check(recs, [b"MM", b"XH", b"RG", b"NM"])
    assert c["malformed_records"] == 8 + 6                 # the newline ones, and the H values of odd length (1, 15, 17, 255, 257, 4097)


@pytest.mark.parametrize("mapping", LANES)
@pytest.mark.parametrize("sub", list("cCsSiI"))
def test_splice_b_counts(lanes, mapping, sub):
    """the 64-element neighbourhoods of the scan step and its carry between steps, values of every digit count"""
    lanes(mapping)
    recs = [T.rec(T.B(b"ML", sub, TC.b_values(sub, n, seed=ord(sub))) + T.Z(b"RG", b"behind"), name=b"b%d" % n)
            for n in (0, 1, 63, 64, 65, 127, 128, 129, 4097)]
    _check(recs, [b"ML", b"RG"])


@pytest.mark.parametrize("mapping", LANES)
def test_splice_a_long_record_next_to_short_ones(lanes, mapping):
    lanes(mapping)
    import random
    rnd = random.Random(3)
    short = [T.rec(T.scalar(b"NM", "i", k) + T.Z(b"RG", b"grp%d" % (k % 3)), name=b"s%d" % k, seq="".join(rnd.choice("ACGT") for _ in range(100))) for k in range(40)]
    mm = (b"C+m," + b",".join(b"%d" % rnd.randrange(0, 30) for _ in range(2000)))[:2047] + b";"
    long_rec = T.rec(T.Z(b"MM", mm) + T.B(b"ML", "C", [rnd.randrange(256) for _ in range(2000)]) + T.Z(b"RG", b"grpL"), name=b"long",
                     seq="".join(rnd.choice("ACGT") for _ in range(10000)))
    _check(short[:20] + [long_rec] + short[20:], [b"MM", b"ML", b"RG"])


@pytest.mark.parametrize("mapping", LANES)
def test_splice_seeded_sweep(lanes, mapping):
    lanes(mapping)
    recs, lst = TC.random_records(5, 2000)
    c = _check(recs, lst)
    assert c["malformed_records"] >= 100 and c["float_values_skipped"] >= 100 and min(c["copied"][:6]) >= 100


def test_splice_fault_contract(lanes):
    lanes(None)
    recs, lst = TC.random_records(9, 300)
    data, text, rs, raw, st = _views(recs)
    want, starts, counts = _want(data, lst)
    assert len(want) > len(text)
    # one byte short: fault 1, the exact size, the counters valid, out untouched
    out, out_start, info = _splice(text, rs, raw, st, lst, cap=len(want) - 1, canary=0x5a)
    assert info[3] == 1 and info[1] == len(want) and (out == 0x5a).all()
    assert info[4] == counts["malformed_records"] and info[5] == counts["float_values_skipped"] and info[8:8 + len(lst)] == counts["copied"]
    # the repeat with info[1]
    out, out_start, info2 = _splice(text, rs, raw, st, lst, cap=info[1], canary=0x5a)
    assert info2[3] == 0 and out[:len(want)].tobytes() == want and out_start == starts and (out[len(want):] == 0x5a).all()
    # a table entry outside its view / a record without '@': fault 2, out untouched
    for which in ("text_end", "raw_end", "raw_back", "text_neg", "no_at", "no_newline"):
        rs2, st2, text2 = list(rs), list(st), bytearray(text)
        if which == "text_end":
            rs2[-1] = len(text) + 1
        elif which == "raw_end":
            st2[-1] = len(raw) + 1
        elif which == "raw_back":
            st2[5] = st2[4] - 1
        elif which == "text_neg":
            rs2[0] = -1
        elif which == "no_at":
            text2[rs[7]] = ord("x")
        else:
            for p in range(rs[9], rs[10]):
                if text2[p] == 0x0a:
                    text2[p] = ord("N")
        out, _, info = _splice(bytes(text2), rs2, raw, st2, lst, canary=0x5a)
        assert info[3] == 2 and (out == 0x5a).all(), which


def test_splice_a_view_that_is_no_view(lanes):
    """table entries that are negative, run backwards or lie far outside the buffers: fault 2 by result, nothing is read or written"""
    import torch
    lanes(None)
    recs = [T.rec(T.Z(b"RG", b"a"), name=b"r%d" % k) for k in range(6)]
    data, text, rs, raw, st = _views(recs)
    for rs2, st2 in ((rs, [0, st[1], st[1] - 1, st[3], 1 << 40, st[4] + 20, st[6]]), ([-5] + rs[1:], st), (rs[:3] + [1 << 41] + rs[4:], st),
                     (rs, [-1 << 40] + st[1:]), ([rs[1]] + [rs[0]] + rs[2:], st)):
        out, _, info = _splice(text, rs2, raw, st2, [b"RG"], canary=0x5a)
        assert info[3] == 2 and info[0] == 0 and info[1] == 0 and (out == 0x5a).all()
    torch.cuda.synchronize()


def test_splice_refuses_bad_arguments():
    from ribodetector_amd import _native as N
    L = N.lib()
    assert L.rd_bam_tag_splice_workspace_bytes(10, 0) == 0 and L.rd_bam_tag_splice_workspace_bytes(10, 17) == 0
    assert L.rd_bam_tag_splice_workspace_bytes(-1, 1) == 0 and L.rd_bam_tag_splice_workspace_bytes(10, 16) > 0
    for tags, n in ((b"R!", 1), (b"1G", 1), (b"RGRG", 2), (b"RG", 0), (b"RG" * 17, 17)):
        rc = L.rd_bam_tag_splice(None, 0, None, None, 0, None, 0, tags, n, None, 0, None, None, None, 0, None)
        assert rc != 0 and b"rd_bam_tag_splice" in L.rd_last_error()


def test_device_bam_tags_repeats_once_on_a_small_hint(monkeypatch):
    """DeviceBamTags.splice over a chunk of the device reader: a hint that is too small costs one more call, the view is the rule's"""
    import torch
    from ribodetector_amd import bamtags
    from ribodetector_amd.data_loader import device_reader as dr
    recs, lst = TC.random_records(21, 500)
    path = os.path.join(_tmpdir(), "hint.bam")
    data = bam.write_bam(path, recs)
    want = bam.fastq_text_tagged(data, lst)
    for hint, repeats in ((None, 0), ("64", 1)):
        if hint is None:
            monkeypatch.delenv(bamtags.HINT_ENV, raising=False)
        else:
            monkeypatch.setenv(bamtags.HINT_ENV, hint)
        tg = bamtags.DeviceBamTags(DEV, lst)
        got = []
        for chunk in dr.get_seq_chunks_device(path, chunk_size=200, device=torch.device(DEV), keep_raw=True):
            chunk.ready.synchronize()
            text, out_start, info = tg.splice(chunk)
            torch.cuda.synchronize()
            got.append(text[:int(info[1])].cpu().numpy().tobytes())
            assert out_start.numel() == chunk.n + 1 and int(out_start[-1]) == int(info[1])
        assert b"".join(got) == want
        assert tg.counts() == bam.tag_counts(data, lst)
        assert (tg.repeats > 0) == bool(repeats)


_TMP = []


def _tmpdir():
    import tempfile
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory(prefix="rd_bamtags_"))
    return _TMP[0].name


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
LIST = [b"RG", b"ML", b"MM", b"NM", b"qs"]
FLAG = ["--bam_tags", "RG,ML,MM,NM,qs"]


def _with_tags(reads):
    for i, r in enumerate(reads):
        if i % 13 == 0:
            continue
        tags = T.Z(b"RG", b"grp%d" % (i % 3)) + T.scalar(b"NM", "i", i - 1500) + T.scalar(b"XS", "A", b"+")
        if i % 5 == 0:
            tags = T.B(b"ML", "C", [(i * 7 + j * 37) % 256 for j in range(i % 40)]) + tags + T.Z(b"MM", b"C+m," + b",".join(b"%d" % (j % 11) for j in range(i % 23)) + b";")
        if i % 17 == 0:
            tags += T.scalar(b"qs", "f", 12.5)
        if i % 29 == 0:
            tags = T.Z(b"RG", b"a\nb") + tags
        if i % 31 == 0:
            tags = tags[:3 + i % 7] if i % 2 else b"XQq\x01" + tags
        r["tags"] = tags
    return reads


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    import test_gpu_bam as G
    import test_interleaved_host as H
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("bamtagsets")
    rng = np.random.default_rng(30)
    out = {}
    a, o, _ = synth.reads_numpy(3000, (60, 150), seed=41, rrna_frac=0.3)
    se = _with_tags(G._bam_reads(a, o, rng=rng))
    se[100] = dict(se[100], flag=0x100 | 0x4)              # a secondary record: skipped, with its tags
    out["se"] = (str(d / "se.bam"), bam.write_bam(str(d / "se.bam"), se, member_bytes=4096))
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(1600, (60, 120), seed=32, rrna_frac=0.3), synth.reads_numpy(1600, (60, 120), seed=33, rrna_frac=0.3)
    r1, r2 = _with_tags(G._bam_reads(a1, o1, mate=1, rng=rng)), _with_tags(G._bam_reads(a2, o2, mate=2, rng=rng))
    for i, r in enumerate(r2):                             # mate 2's tags differ from mate 1's
        if "tags" in r and i % 3 == 0:
            r["tags"] = T.scalar(b"NM", "C", i % 200)
    out["m1"] = (str(d / "m1.bam"), bam.write_bam(str(d / "m1.bam"), r1))
    out["m2"] = (str(d / "m2.bam"), bam.write_bam(str(d / "m2.bam"), r2))
    out["il"] = (str(d / "il.bam"), bam.write_bam(str(d / "il.bam"), H.interleave(r1, r2)))
    return out


def _by_name(data, tags=LIST):
    out = {}
    for r in bam.records(data):
        if not r.skipped:
            t = r.fastq()
            at = t.index(b"\n")
            assert t[1:at] not in out
            out[t[1:at]] = t[:at] + bam.tag_comment(data, r.offset, tags)[0] + t[at:]
    assert b"".join(out.values()) == bam.fastq_text_tagged(data, tags)
    return out


def _expect(plain, by_name):
    """the tagged text of the records a run without the flag selected (their names, in the file's order)"""
    lines = plain.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return b"".join(by_name[lines[i][1:]] for i in range(0, len(lines) - 1, 4))


def _read(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if path.endswith("gz") else raw


def _two_runs(caplog, tmp_path, inputs, names, extra=(), env=None, flag=FLAG, also=()):
    """the same arguments without and with the flag: ({name: bytes} of each run, the log of the flagged run, its Predictor)"""
    import logging
    import test_gpu_bam as G
    caplog.set_level(logging.INFO)
    res = []
    for tag, fl in (("base", []), ("tags", list(flag))):
        d = tmp_path / tag
        d.mkdir()
        caplog.clear()
        args = ["-l", "100", "-i", *inputs]
        for opt, files in names:
            args += [opt] + [str(d / f) for f in files]
        args += list(extra) + fl + G.SMALL
        p = G._run(args, env=env)
        files = {f: _read(str(d / f)) for _, fs in names for f in fs}
        for f in also:
            files[f] = _read(str(d / f)) if os.path.exists(str(d / f)) else None
        res.append((files, caplog.text, p))
    return res[0][0], res[1][0], res[1][1], res[1][2]


def _log_counts(log, tags=LIST):
    import re
    m = re.search(r"BAM tags: (.*) copied; (\d+) records with malformed tags, (\d+) float values skipped", log)
    assert m, log[-2000:]
    got = [x.split(" ") for x in m.group(1).split(", ")]
    assert [g[0].encode() for g in got] == list(tags)
    return {"copied": [int(g[1]) for g in got], "malformed_records": int(m.group(2)), "float_values_skipped": int(m.group(3))}


@pytest.mark.parametrize("gz_out", [False, True])
def test_cli_single_end(caplog, tmp_path, sets, gz_out):
    path, data = sets["se"]
    ext = ".fq.gz" if gz_out else ".fq"
    base, tagged, log, p = _two_runs(caplog, tmp_path, [path], [("-o", ["o" + ext]), ("-r", ["r" + ext])])
    names = _by_name(data)
    assert p.num_read == 2999 and p.ingest["se.bam"]["indexer"]["bam_records"] == 3000 and min(len(base["o" + ext]), len(base["r" + ext])) > 1000
    for f in base:
        assert tagged[f] == _expect(base[f], names) and tagged[f] != base[f], f
    want = bam.tag_counts(data, LIST)
    assert _log_counts(log) == want and min(want["copied"][:4]) > 50 and want["copied"][4] == 0         # (qs is float-typed: counted, not copied)
    assert want["malformed_records"] > 50 and want["float_values_skipped"] > 50
    assert p.num_read > 2 * 1024                           # (chunks of 1,024 reads: three of them)


def test_cli_two_files_ensure_both(caplog, tmp_path, sets):
    (p1, d1), (p2, d2) = sets["m1"], sets["m2"]
    unc = ["o1.fq.unclassified.gz", "o2.fq.gz.unclassified.gz"]
    base, tagged, log, p = _two_runs(caplog, tmp_path, [p1, p2], [("-o", ["o1.fq", "o2.fq.gz"]), ("-r", ["r1.fq.gz", "r2.fq"])],
                                     extra=["-e", "both", "--summary", "PATH"], also=unc)
    n1, n2 = _by_name(d1), _by_name(d2)
    assert p.is_paired and all(base[f] is not None and len(base[f]) > 0 for f in base)
    for f in base:
        assert tagged[f] == _expect(base[f], n1 if "1" in f.split(".")[0] else n2), f
    w1, w2 = bam.tag_counts(d1, LIST), bam.tag_counts(d2, LIST)
    got = _log_counts(log)
    assert got["copied"] == [a + b for a, b in zip(w1["copied"], w2["copied"])] and got["malformed_records"] == w1["malformed_records"] + w2["malformed_records"]


@pytest.mark.parametrize("outs", [1, 2])
def test_cli_interleaved(caplog, tmp_path, sets, outs):
    path, data = sets["il"]
    o = ["o%d.fq.gz" % k for k in range(outs)]
    r = ["r%d.fq" % k for k in range(outs)]
    base, tagged, log, p = _two_runs(caplog, tmp_path, [path], [("-o", o), ("-r", r)], extra=["--interleaved", "-e", "both"], also=[x + ".unclassified.gz" for x in o])
    names = _by_name(data)
    assert p.is_paired and p.num_read == 1600        # (chunks of 512 pairs: four of them)
    for f in base:
        assert base[f] is not None and tagged[f] == _expect(base[f], names), f
    assert _log_counts(log) == bam.tag_counts(data, LIST)


def test_cli_host_gzip(caplog, tmp_path, sets):
    path, data = sets["se"]
    base, tagged, log, p = _two_runs(caplog, tmp_path, [path], [("-o", ["o.fq.gz"]), ("-r", ["r.fq"])], env={"RD_DEVICE_GZIP": "host"})
    names = _by_name(data)
    for f in base:
        assert tagged[f] == _expect(base[f], names) and tagged[f] != base[f], f


def test_cli_everything_else_sees_the_untagged_view(caplog, tmp_path, sets):
    """--windows --regions --read_report --summary together: the report, the regions and the summary do not change with the flag, apart
    from the summary's "bam_tags" key; the outputs carry the tags"""
    path, data = sets["se"]
    side = ["rep.tsv", "regions.bed", "s.json"]
    base, tagged, log, p = _two_runs(caplog, tmp_path, [path], [("-o", ["o.fq"]), ("-r", ["r.fq.gz"]), ("--read_report", side[:1]), ("--regions", side[1:2]),
                                                        ("--summary", side[2:])], extra=["--windows"])
    names = _by_name(data)
    for f in ("o.fq", "r.fq.gz"):
        assert tagged[f] == _expect(base[f], names) and tagged[f] != base[f], f
    assert tagged["rep.tsv"] == base["rep.tsv"] and tagged["regions.bed"] == base["regions.bed"] and len(base["regions.bed"]) > 100
    db, dt = json.loads(base["s.json"]), json.loads(tagged["s.json"])
    got = dt.pop("bam_tags")
    assert "bam_tags" not in db and dt == db
    want = bam.tag_counts(data, LIST)
    assert got == {"tags": [t.decode() for t in LIST], "copied": want["copied"], "malformed_records": want["malformed_records"],
                   "float_values_skipped": want["float_values_skipped"]}
    i = tagged["s.json"].index(b'"bam_tags"')
    assert base["s.json"][:i - 10] == tagged["s.json"][:i - 10]           # (the key stands at the end: what is in front of it is the same bytes)


def test_cli_summary_of_two_files_counts_per_mate(tmp_path, sets):
    import test_gpu_bam as G
    (p1, d1), (p2, d2) = sets["m1"], sets["m2"]
    s = str(tmp_path / "s.json")
    G._run(["-l", "100", "-i", p1, p2, "-o", str(tmp_path / "o1.fq"), str(tmp_path / "o2.fq"), "--summary", s] + FLAG + G.SMALL)
    got = json.load(open(s))["bam_tags"]
    w = [bam.tag_counts(d, LIST) for d in (d1, d2)]
    assert got["copied"] == [[w[0]["copied"][j], w[1]["copied"][j]] for j in range(len(LIST))]
    assert got["malformed_records"] == [x["malformed_records"] for x in w] and got["float_values_skipped"] == [x["float_values_skipped"] for x in w]


def test_cli_tags_that_no_record_carries(caplog, tmp_path, sets):
    """the outputs are the bytes of the run without the flag, the .gz file's too"""
    path, data = sets["se"]
    import logging
    import test_gpu_bam as G
    res = {}
    caplog.set_level(logging.INFO)
    for tag, fl in (("base", []), ("tags", ["--bam_tags", "ZZ,Y1"])):
        d = tmp_path / tag
        d.mkdir()
        G._run(["-l", "100", "-i", path, "-o", str(d / "o.fq.gz"), "-r", str(d / "r.fq")] + fl + G.SMALL)
        res[tag] = [open(str(d / f), "rb").read() for f in ("o.fq.gz", "r.fq")]
    assert res["base"] == res["tags"] and len(res["base"][0]) > 1000
    assert _log_counts(caplog.text, [b"ZZ", b"Y1"])["copied"] == [0, 0]


def test_cli_two_ranks_bam_shard(caplog, tmp_path, sets):
    """two ranks under --bam_shard: the joined outputs equal one rank's, the log and the summary hold the sums"""
    import logging
    import test_gpu_bam as G
    import test_gpu_cli as CLI
    path, data = sets["se"]
    runs = {}
    for tag, world in (("one", 1), ("two", 2)):
        d = tmp_path / tag
        d.mkdir()
        files = [str(d / x) for x in ("o.fq", "r.fq.gz", "s.json")]
        args = ["-l", "100", "-i", path, "-o", files[0], "-r", files[1], "--summary", files[2], "--bam_shard"] + FLAG + G.SMALL
        if world == 1:
            caplog.set_level(logging.INFO)
            G._run(args)
            log = caplog.text
        else:
            r, _ = CLI._torchrun(world, args, timeout=600)
            log = r.stdout + r.stderr
            assert r.returncode == 0, log[-3000:]
            assert len(set(__import__("re").findall(r"Rank (\d) parses", log))) == 2
        runs[tag] = [_read(files[0]), _read(files[1]), json.load(open(files[2]))["bam_tags"], _log_counts(log)]
    assert runs["one"] == runs["two"]
    want = bam.tag_counts(data, LIST)
    assert runs["two"][3] == want and runs["two"][2]["copied"] == want["copied"]
