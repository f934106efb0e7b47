"""--ubam_tags on the GPU. Kernel tests: rd_bam_encode_ex (csrc/rd_bam_encode.hpp) through ubam.encode(..., tags=...) on chunks built
here, into a buffer with the guard bytes and fill of tests/test_gpu_ubam.py - raw, raw_start and all of info compared with the rule
(bam.from_fastq(tags=), ubam_counts, ubam_tag_counts) byte for byte. CLI tests: the same command without the flags (FASTQ outputs) and
with them; every .bam inflated and held against the header plus bam.from_fastq(text output, tags=).

Launch shapes: the tag passes give a record L = 4 or 16 lanes (RD_TAG_LANES forces either; the call chooses 16 when the mean record
of the text is 1,024 bytes or longer), 256 threads per workgroup; a step of a search or of a B array is 16 L bytes."""
import json
import logging
import os
import random
import struct

import numpy as np
import pytest

import test_gpu_ubam as U
import ubam_tags_cases as UT
from ribodetector_amd import _native as N
from ribodetector_amd import bam

pytestmark = pytest.mark.gpu

DEV = U.DEV
NAMES = [b"MM", b"ML", b"RG", b"XI"]


def _encode(text, rs, so, sl, n, flags, names, raw_cap=None):
    """one call on the device; returns (raw buffer with its guard as numpy, raw_start, info)"""
    import torch
    from ribodetector_amd import ubam
    cap = 3 * len(text) + 64 * n + 64 if raw_cap is None else raw_cap          # (ample: the bound plus twice the text)
    raw = torch.full((((cap + 15) // 16) * 16 + U.GUARD,), U.FILL, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV)
    tabs = [torch.from_numpy(x).to(DEV) for x in (rs, so, sl)]
    _, raw_start, info = ubam.encode(t, *tabs, n, flags, raw_cap=cap, raw=raw, text_bytes=len(text), tags=names)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), raw_start.cpu().numpy(), info.cpu().numpy()


def _sizes(want, n):
    sizes, p = [], 0
    while p < len(want):
        sizes.append(struct.unpack_from("<i", want, p)[0] + 4)
        p += sizes[-1]
    assert len(sizes) == n
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def _check(records, names, n_mates=1, mate=0, fasta=False, raw_cap=None):
    """encode the records and hold everything against the rule"""
    from ribodetector_amd import ubam
    text, rs, so, sl = U._chunk(records, fasta)
    n = len(records)
    want = bam.from_fastq(text, n_mates, mate, fasta, tags=names)
    got, raw_start, info = _encode(text, rs, so, sl, n, ubam.flags_word(n_mates, mate, fasta), names, raw_cap)
    c, tc = bam.ubam_counts(text, n_mates, mate, fasta), bam.ubam_tag_counts(text, names, fasta)
    assert info.tolist() == [n, len(want), -1, 0, c["bases_changed"], c["quals_clamped"], c["names_starred"], -1, tc["malformed_records"],
                             tc["float_values_skipped"]] + tc["copied"], (info, c, tc)
    assert np.array_equal(raw_start, _sizes(want, n))
    if got[:len(want)].tobytes() != want:
        bad = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
        k = int(np.searchsorted(raw_start, bad[0], side="right")) - 1
        raise AssertionError("raw differs at %d bytes, first %d (record %d, byte %d of %d) last %d of %d" % (
            len(bad), bad[0], k, bad[0] - raw_start[k], raw_start[k + 1] - raw_start[k], bad[-1], len(want)))
    assert (got[len(want):] == U.FILL).all(), "bytes written behind the records"
    return want, raw_start, tc


def _rec(head, l_seq=4, k=0):
    return (head, (b"ACGTN" * (l_seq // 5 + 1))[:l_seq], bytes(40 + (k + i) % 30 for i in range(l_seq)))


@pytest.fixture(params=["4", "16"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("RD_TAG_LANES", request.param)
    return int(request.param)


def test_the_case_table(lanes):
    cases = [c for c in UT.CASES if c[1].startswith(b"@")]
    heads = [c[1][1:].split(b"\n")[0] for c in cases]
    # every case with its own names, against what the table says by hand: one chunk per list of names
    groups = {}
    for c, h in zip(cases, heads):
        groups.setdefault(tuple(c[2]), []).append((c, h))
    for names, members in groups.items():
        want, raw_start, _ = _check([_rec(h, 3 + k % 5, k) for k, (_, h) in enumerate(members)], list(names))
        for k, (c, h) in enumerate(members):
            tags = UT.expected(c)[0]
            r = want[raw_start[k]:raw_start[k + 1]]
            assert r.endswith(tags) and len(r) == 36 + len(bam.ubam_name(b"@" + h)) + 1 + (3 + k % 5 + 1) // 2 + 3 + k % 5 + len(tags), c[0]
    # the whole table as one chunk, 16 names listed
    _, _, tc = _check([_rec(h, k % 7, k) for k, h in enumerate(heads)], [b"MM", b"ML", b"RG", b"XI", b"X0"] + [b"X%c" % c for c in b"PONMLKJHGFE"])
    assert tc["malformed_records"] > 30 and tc["float_values_skipped"] >= 3


def test_comment_lengths_on_every_residue(lanes):
    records = []
    for c in range(0, 140):
        name = b"n" * (1 + c % 3)
        value = bytes(33 + (c + i) % 90 for i in range(c))
        head = name + (b"\t" if c % 2 else b" ") + b"RG:Z:" + value                 # a comment of 5 + c bytes
        records.append(_rec(head, c % 16 + (16 if c % 7 == 0 else 0), c))
        if c % 3 == 0:
            records.append(_rec(name + b"\tXX:Z:skip\tRG:Z:" + value + b"\tXI:i:%d" % (c * 997), c % 5, c))
    want, raw_start, tc = _check(records, NAMES)
    assert tc["copied"][2] == len(records) and tc["copied"][3] == 47
    comments = {len(bam.ubam_comment(b"@" + r[0])) % 64 for r in records}
    assert comments == set(range(64))
    tag_at = {(int(raw_start[k + 1]) - len(bam.tags_from_comment(b"@" + r[0], NAMES)[0])) % 16 for k, r in enumerate(records)}
    assert tag_at == set(range(16)), "the tag bytes start on every residue modulo 16"


def _array(rng, sub, count):
    lo, hi = UT.B_RANGE[sub]
    vals = rng.integers(lo, hi, count, endpoint=True).tolist()
    for i in range(0, count, 3):                                   # short elements too: one digit, a sign, a leading zero
        vals[i] = (0, 7, hi, lo)[(i // 3) % 4]
    return b"ML:B:" + sub.encode() + b"".join((b",+%d" if i % 11 == 5 and v >= 0 else b",0%d" if i % 13 == 6 and 0 <= v < 10 ** 9 else b",%d") % v
                                              for i, v in enumerate(vals))


def test_b_arrays_around_the_lane_count(lanes):
    rng = np.random.default_rng(21)
    records = []
    for sub in "cCsSiI":
        for count in (lanes - 1, lanes, lanes + 1, 4 * lanes + 1):
            records.append(_rec(b"a%d%s\t" % (count, sub.encode()) + _array(rng, sub, count) + b"\tRG:Z:behind", count % 9, count))
    records.append(_rec(b"big\tMM:Z:C+m?" + b",1" * 700 + b";\t" + _array(rng, "C", 2000) + b"\tRG:Z:x", 50))
    records.append(_rec(b"bigs\t" + _array(rng, "s", 2000), 7))
    records.append(_rec(b"bad\t" + _array(rng, "C", 300) + b",256", 7))       # the last element out of range: no tags
    _, _, tc = _check(records, NAMES)
    assert tc["malformed_records"] == 1 and tc["copied"][1] == len(records) - 1


def test_an_array_of_25000_elements_between_short_records():
    rng = np.random.default_rng(22)
    short = [_rec(b"s%d\tRG:Z:lib%d\tML:B:C,1,2,%d" % (i, i, i), 20 + i, i) for i in range(40)]
    big = (b"big\tMM:Z:C+m?" + b",0" * 25000 + b";\t" + _array(rng, "C", 25000) + b"\tRG:Z:lib7", b"ACGT" * 2500, b"I" * 10000)
    assert len(big[0]) > 100000
    want, raw_start, tc = _check(short[:20] + [big] + short[20:], NAMES)
    assert raw_start[21] - raw_start[20] > 5 * 16384, "the record spans several tiles of the write pass"
    assert tc["copied"] == [1, 41, 41, 0]


def _sweep(n, seed):
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        fields = [UT.random_field(rnd) for _ in range(rnd.randrange(0, 5))]
        sep = (b" ", b"\t", b"\t", b"")[k % 4]
        head = b"r%d" % k + (sep + b"\t".join(fields) if sep else b"") + (b"\r" if k % 97 == 0 else b"")
        ls = rnd.randrange(0, 60)
        out.append((head, bytes(rnd.choice(b"ACGTN") for _ in range(ls)), bytes(rnd.randrange(33, 75) for _ in range(ls))))
    return out


def test_sweep_of_20000_records():
    records = _sweep(20000, 23)
    _, _, tc = _check(records, NAMES)
    assert min(tc["copied"]) > 500 and tc["malformed_records"] > 500 and tc["float_values_skipped"] > 100


def test_no_names_is_rd_bam_encode_bit_for_bit():
    import torch
    from ribodetector_amd import ubam
    records = U._sweep_records(5000, 7)
    text, rs, so, sl = U._chunk(records)
    n, lib, flags = len(records), N.lib(), ubam.flags_word()
    a_raw, a_start, a_info = U._encode(text, rs, so, sl, n, flags)
    assert a_info[3] == 0 and a_raw[:int(a_info[1])].tobytes() == bam.from_fastq(text)
    cap = bam.ubam_bound(len(text), n)
    raw = torch.full((((cap + 15) // 16) * 16 + U.GUARD,), U.FILL, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV)
    tabs = [torch.from_numpy(x).to(DEV) for x in (rs, so, sl)]
    raw_start = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    info = torch.full((12,), -7, dtype=torch.int64, device=DEV)
    assert lib.rd_bam_encode_tags_workspace_bytes(n, 0) == lib.rd_bam_encode_workspace_bytes(n)
    ws = torch.empty(int(lib.rd_bam_encode_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        N.check(lib.rd_bam_encode_ex(N.ptr(t), len(text), *(N.ptr(x) for x in tabs), n, 0, 1, flags, None, 0, N.ptr(raw), cap, N.ptr(raw_start), N.ptr(info),
                                     N.ptr(ws), ws.numel(), N.stream_ptr(torch.device(DEV))), "rd_bam_encode_ex")
    torch.cuda.synchronize()
    assert np.array_equal(raw.cpu().numpy(), a_raw) and np.array_equal(raw_start.cpu().numpy(), a_start)
    assert info.cpu().numpy().tolist() == a_info.tolist() + [-7] * 4, "eight words of info, nothing behind them"
    # records without a comment, names listed: the same bytes again
    got, start, tinfo = _encode(text, rs, so, sl, n, flags, [b"ZQ"], raw_cap=cap)
    assert got.tobytes() == a_raw.tobytes() and np.array_equal(start, a_start) and tinfo.tolist() == a_info.tolist() + [0, 0, 0]
    # the library refuses what is no list of names
    args = (N.ptr(t), len(text), *(N.ptr(x) for x in tabs), n, 0, 1, flags)
    tail = (N.ptr(raw), cap, N.ptr(raw_start), N.ptr(info), N.ptr(ws), ws.numel(), None)
    for names, k in ((b"MMMM", 2), (b"1M", 1), (b"MM" * 17, 17), (None, 1)):
        assert lib.rd_bam_encode_ex(*args, names, k, *tail) != 0
    assert lib.rd_bam_encode_tags_workspace_bytes(n, 17) == 0 and lib.rd_bam_encode_tags_workspace_bytes(n, 3) > lib.rd_bam_encode_workspace_bytes(n)


def test_raw_cap_one_byte_short():
    from ribodetector_amd import ubam
    records = _sweep(3000, 24)
    text, rs, so, sl = U._chunk(records)
    want = bam.from_fastq(text, tags=NAMES)
    got, raw_start, info = _encode(text, rs, so, sl, len(records), ubam.flags_word(), NAMES, raw_cap=len(want) - 1)
    assert info[3] == 1 and info[0] == 0 and info[1] == len(want), "fault 1 and the exact need"
    assert (got == U.FILL).all(), "written although the records do not fit"
    assert (raw_start == 0).all()
    _check(records, NAMES, raw_cap=int(info[1]))
    # a header line that does not end inside its record: a status, nothing written
    bad = rs.copy()
    bad[101] = bad[100] + 2
    got, raw_start, info = _encode(text, bad, so, sl, len(records), ubam.flags_word(), NAMES)
    assert info[3] == 2 and info[1] == 0 and (got == U.FILL).all() and (raw_start == 0).all() and (info[8:] == 0).all()
    # no records
    got, raw_start, info = _encode(b"\n" * 16, np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), 0, ubam.flags_word(), NAMES)
    assert info.tolist() == [0, 0, -1, 0, 0, 0, 0, -1] + [0] * 6 and raw_start.tolist() == [0] and (got == U.FILL).all()


def test_interleaved_and_mate_files():
    records = []
    for i in range(1500):
        t1, t2 = ((b"/1", b"/2"), (b"", b""), (b"/2", b"/1"))[i % 3]
        records.append(_rec(b"p%d" % i + t1 + b"\tRG:Z:one%d\tXI:i:%d" % (i, i), i % 50, i))
        records.append(_rec(b"p%d" % i + t2 + b" MM:Z:two\tML:B:S,%d,1" % i, (i * 7) % 50, i))
    want, _, tc = _check(records, NAMES, n_mates=2, mate=bam.INTERLEAVED)
    assert tc["copied"] == [1500, 1500, 1500, 1500]
    recs = list(bam.records(want, 0))
    assert recs[0].name == recs[1].name == b"p0" and (recs[0].flag, recs[1].flag) == (77, 141)
    for mate in (0, 1):
        _check(records[mate::2], NAMES, n_mates=2, mate=mate)      # each mate takes the tags of its own header line


def test_fasta():
    rng = np.random.default_rng(25)
    records = [(b"s%d RG:Z:fa%d\tML:B:c,-1,%d" % (i, i, i % 100), U._seq(rng, int(rng.integers(1, 300)), b"ACGTNRY"), None) for i in range(3000)]
    records += [(b"", b"ACGT", None), (b"long\tXI:A:q", U._seq(rng, 40001), None)]
    _, _, tc = _check(records, NAMES, fasta=True)
    assert tc["copied"] == [0, 3000, 3000, 1]


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
LIST = "MM,ML,RG"
CLI_NAMES = [b"MM", b"ML", b"RG"]


def _comment(i, rng):
    """what a modified-base caller leaves behind a read name - for some reads nothing, an Illumina comment, a float, a malformed tag"""
    n = int(rng.integers(0, 12))
    full = b"\tMM:Z:C+m?" + b"".join(b",%d" % v for v in rng.integers(0, 9, n)) + b";\tML:B:C" + b"".join(b",%d" % v for v in rng.integers(0, 256, n)) + b"\tRG:Z:lib%d" % (i % 3)
    return (full, full, full, b" 1:N:0:ACGT", b"", b"\tRG:Z:only", b"\tqs:f:11.5\tML:B:f,0.5,1\tRG:Z:lib1", b"\tML:B:C,300\tRG:Z:lib2", b" RG:Z:behind a space", full)[i % 10]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import gzip
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("ubamtags")
    out = {}

    def write(path, arena, off, mate):
        raw, rng = arena.tobytes(), np.random.default_rng(len(off) + mate)
        with (gzip.open if path.endswith("gz") else open)(path, "wb") as fh:
            for i in range(len(off) - 1):
                s = raw[off[i]:off[i + 1]]
                q = bytes(rng.integers(33, 75, len(s), dtype=np.uint8))
                fh.write(b"@syn.%d" % i + (b"/%d" % mate if mate and i % 3 else b"") + _comment(i + mate, rng) + b"\n" + s + b"\n+\n" + q + b"\n")
        return path
    a, o, _ = synth.reads_numpy(2500, (60, 120), seed=51, rrna_frac=0.3)
    out["se"] = write(str(d / "se.fq"), a, o, 0)
    (a1, o1, _), (a2, o2, _) = synth.reads_numpy(1300, (60, 120), seed=52, rrna_frac=0.3), synth.reads_numpy(1300, (60, 120), seed=53, rrna_frac=0.3)
    out["m1"], out["m2"] = write(str(d / "m1.fq.gz"), a1, o1, 1), write(str(d / "m2.fq.gz"), a2, o2, 2)
    with open(str(d / "il.fq"), "wb") as fh:
        r1, r2 = U._read(out["m1"]).split(b"\n"), U._read(out["m2"]).split(b"\n")
        for k in range(0, len(r1) - 1, 4):
            fh.write(b"\n".join(r1[k:k + 4] + r2[k:k + 4]) + b"\n")
    out["il"] = str(d / "il.fq")
    return out


def _both_runs(caplog, tmp_path, inputs, outs, extra=(), env=None, mates=None, unclassified=False):
    """the same command without the flags and with them; returns the flagged run, its summary and its log"""
    n_mates = 1 if mates is None else 2
    res = {}
    for flag in (False, True):
        d = tmp_path / ("ubam" if flag else "text")
        d.mkdir()
        ext = ".bam" if flag else ".fq"
        o, r = [str(d / ("o%d%s" % (k, ext))) for k in range(outs)], [str(d / ("r%d%s" % (k, ext))) for k in range(outs)]
        summ = str(d / "summary.json")
        caplog.clear()
        with caplog.at_level(logging.INFO):
            p = U._run(["-l", "100", "-i", *inputs, "-o", *o, "-r", *r, "--summary", summ, *extra] + (["--ubam_output", "--ubam_tags", LIST] if flag else []) + U.SMALL,
                       env if flag else None)
        files = {os.path.basename(x)[:2]: x for x in o + r}
        if unclassified:
            files.update({"u%d" % k: x + (".unclassified.bam" if flag else ".unclassified.gz") for k, x in enumerate(o)})
        res[flag] = (p, files, open(summ, "rb").read(), caplog.text)
    (p0, f0, raw0, log0), (p1, f1, raw1, log1) = res[False], res[True]
    assert "BAM tags from text" not in log0
    assert (p0.num_read, p0.num_nonrrna, p0.num_rrna, p0.num_unknown) == (p1.num_read, p1.num_nonrrna, p1.num_rrna, p1.num_unknown)
    s1 = json.loads(raw1)
    assert list(s1)[-2:] == ["ubam_output", "ubam_tags"] and "ubam_tags" not in json.loads(raw0)
    assert raw1[:raw1.index(b',\n "ubam_output": ')] + b"\n}\n" == raw0, "the summary minus the new keys is the same bytes"
    tagged = 0
    for key in f0:
        text = U._read(f0[key])
        k = int(key[1])
        mate = 0 if mates is None else bam.INTERLEAVED if mates == "interleaved" and outs == 1 else k
        data = U._inflate_bam(f1[key])
        assert data == U.HEADER + bam.from_fastq(text, n_mates, mate, tags=CLI_NAMES), key
        tagged += len(data) - len(U.HEADER) - len(bam.from_fastq(text, n_mates, mate))
    assert tagged > 10000, "the outputs carry tags"
    return p1, s1["ubam_tags"], log1


def _counted(paths):
    return [bam.ubam_tag_counts(U._read(p), CLI_NAMES) for p in paths]


def _check_counters(got, log, per_file):
    from ribodetector_amd import ubam
    assert got == ubam.to_json_tags(CLI_NAMES, per_file)
    assert ubam.log_line_tags(CLI_NAMES, per_file) in log and "BAM tags from text: MM " in log
    assert sum(c["malformed_records"] for c in per_file) > 0 and sum(c["float_values_skipped"] for c in per_file) > 0


def test_cli_single_end(tmp_path, inputs, caplog):
    p, got, log = _both_runs(caplog, tmp_path, [inputs["se"]], 1)
    assert p.num_read == 2500 and p._ubam[0].repeats == 0
    _check_counters(got, log, _counted([inputs["se"]]))
    assert got["copied"][2] > got["copied"][0] > 0 and isinstance(got["malformed_records"], int)


def test_cli_two_files_gz(tmp_path, inputs, caplog):
    p, got, log = _both_runs(caplog, tmp_path, [inputs["m1"], inputs["m2"]], 2, extra=["-e", "rrna"], mates="files")
    assert p.is_paired and p.num_read == 1300
    _check_counters(got, log, _counted([inputs["m1"], inputs["m2"]]))
    assert all(len(x) == 2 for x in got["copied"]) and len(got["malformed_records"]) == 2, "each count is [mate 1's, mate 2's]"


@pytest.mark.parametrize("outs", [1, 2])
def test_cli_interleaved(tmp_path, inputs, outs, caplog):
    p, got, log = _both_runs(caplog, tmp_path, [inputs["il"]], outs, extra=["--interleaved"], mates="interleaved")
    assert p.num_read == 1300
    _check_counters(got, log, _counted([inputs["il"]]))


def test_cli_ensure_both(tmp_path, inputs, caplog):
    p, got, log = _both_runs(caplog, tmp_path, [inputs["m1"], inputs["m2"]], 2, extra=["-e", "both"], mates="files", unclassified=True)
    _check_counters(got, log, _counted([inputs["m1"], inputs["m2"]]))


def test_cli_a_chunk_through_the_retry(tmp_path, inputs, caplog):
    p, got, log = _both_runs(caplog, tmp_path, [inputs["se"]], 1, env={"RD_UBAM_TAGS_HINT": "1"})
    assert p._ubam[0].repeats >= 2, "every chunk is encoded a second time, at the size the first call reported"
    _check_counters(got, log, _counted([inputs["se"]]))


def test_cli_the_flag_without_ubam_output(tmp_path, inputs):
    with pytest.raises(RuntimeError, match="--ubam_tags .* give --ubam_output with it"):
        U._run(["-l", "100", "-i", inputs["se"], "-o", str(tmp_path / "o.fq"), "--ubam_tags", LIST] + U.SMALL)
    with pytest.raises(RuntimeError, match="--ubam_tags: .*not a tag name"):
        U._run(["-l", "100", "-i", inputs["se"], "-o", str(tmp_path / "o.bam"), "--ubam_output", "--ubam_tags", "MM,M"] + U.SMALL)
    assert not os.path.exists(str(tmp_path / "o.fq")) and not os.path.exists(str(tmp_path / "o.bam"))


def test_cli_round_trip(tmp_path):
    """tagged FASTQ -> --ubam_output --ubam_tags -> -i out.bam --bam_tags: the header lines come back"""
    from ribodetector_amd import synth
    a, o, _ = synth.reads_numpy(600, (60, 120), seed=54, rrna_frac=0.3)
    raw, rng = a.tobytes(), np.random.default_rng(54)
    src, heads = str(tmp_path / "in.fq"), []
    with open(src, "wb") as fh:
        for i in range(len(o) - 1):
            s = raw[o[i]:o[i + 1]]
            n = int(rng.integers(0, 20))
            heads.append(b"@syn.%d" % i + (b"\tMM:Z:C+m?" + b"".join(b",%d" % v for v in rng.integers(0, 9, n)) + b";\tML:B:C" +
                                           b"".join(b",%d" % v for v in rng.integers(0, 256, n)) if i % 4 else b"") + b"\tRG:Z:lib%d" % (i % 3))
            fh.write(heads[-1] + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    ob, rb = str(tmp_path / "o.bam"), str(tmp_path / "r.bam")
    p = U._run(["-l", "100", "-i", src, "-o", ob, "-r", rb, "--ubam_output", "--ubam_tags", LIST] + U.SMALL)
    assert p.num_read == 600
    back = []
    for k, path in enumerate((ob, rb)):
        o2, r2 = str(tmp_path / ("o%d.fq" % k)), str(tmp_path / ("r%d.fq" % k))
        U._run(["-l", "100", "-i", path, "-o", o2, "-r", r2, "--bam_tags", LIST] + U.SMALL)
        back += U._read(o2).split(b"\n")[0::4] + U._read(r2).split(b"\n")[0::4]
    assert sorted(h for h in back if h) == sorted(heads)
