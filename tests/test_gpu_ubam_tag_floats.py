"""--ubam_tag_floats on the GPU. Kernel tests: rd_bam_encode_ex with RD_UBAM_TAG_FLOATS (the FLOATS = true instances of the two tag
kernels, csrc/rd_bam_encode.hpp, with the converter of csrc/rd_float_parse.hpp) through ubam.encode(..., tags=, floats=True), into a
buffer with guard bytes - raw, raw_start and all of info compared with the rule (bam.from_fastq(tags=, floats=True), ubam_counts,
ubam_tag_counts(floats=True)) byte for byte. CLI tests: the flag through detect.main, and BAM -> tagged FASTQ -> BAM -> tagged FASTQ.

Launch shapes: the tag passes give a record L = 4 or 16 lanes (RD_TAG_LANES forces either), 256 threads per workgroup; a step of a B
array is 16 L bytes of its text, a lane scans the elements whose comma stands in its 16."""
import json
import logging
import random
import struct

import numpy as np
import pytest

import bam_float_cases as F
import bam_tags_cases as BT
import float_parse_cases as C
import test_gpu_ubam as U
import ubam_tag_float_cases as UF
import ubam_tags_cases as UT
from ribodetector_amd import _native as N
from ribodetector_amd import bam

pytestmark = pytest.mark.gpu

DEV = U.DEV
NAMES = [b"qs", b"XF", b"RG", b"ML", b"NM"]
LONG = UF.LONG


def _encode(text, rs, so, sl, n, flags, names, raw_cap=None, floats=True):
    import torch
    from ribodetector_amd import ubam
    cap = 3 * len(text) + 64 * n + 64 if raw_cap is None else raw_cap
    raw = torch.full((((cap + 15) // 16) * 16 + U.GUARD,), U.FILL, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV)
    tabs = [torch.from_numpy(x).to(DEV) for x in (rs, so, sl)]
    _, raw_start, info = ubam.encode(t, *tabs, n, flags, raw_cap=cap, raw=raw, text_bytes=len(text), tags=names, floats=floats)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), raw_start.cpu().numpy(), info.cpu().numpy()


def _sizes(want, n):
    sizes, p = [], 0
    while p < len(want):
        sizes.append(struct.unpack_from("<i", want, p)[0] + 4)
        p += sizes[-1]
    assert len(sizes) == n
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def _check(records, names, raw_cap=None):
    """encode the records with the bit set and hold everything against the rule"""
    from ribodetector_amd import ubam
    text, rs, so, sl = U._chunk(records)
    n = len(records)
    want = bam.from_fastq(text, tags=names, floats=True)
    got, raw_start, info = _encode(text, rs, so, sl, n, ubam.flags_word(), names, raw_cap)
    c, tc = bam.ubam_counts(text), bam.ubam_tag_counts(text, names, floats=True)
    assert info.tolist() == [n, len(want), -1, 0, c["bases_changed"], c["quals_clamped"], c["names_starred"], -1, tc["malformed_records"],
                             tc["float_values_skipped"]] + tc["copied"], (info, c, tc)
    assert np.array_equal(raw_start, _sizes(want, n))
    if got[:len(want)].tobytes() != want:
        bad = np.flatnonzero(got[:len(want)] != np.frombuffer(want, np.uint8))
        k = int(np.searchsorted(raw_start, bad[0], side="right")) - 1
        raise AssertionError("raw differs at %d bytes, first %d (record %d %r, byte %d of %d)" % (
            len(bad), bad[0], k, records[k][0][:80], bad[0] - raw_start[k], raw_start[k + 1] - raw_start[k]))
    assert (got[len(want):] == U.FILL).all(), "bytes written behind the records"
    return want, raw_start, tc


def _rec(head, l_seq=4, k=0):
    return (head, (b"ACGTN" * (l_seq // 5 + 1))[:l_seq], bytes(40 + (k + i) % 30 for i in range(l_seq)))


@pytest.fixture(params=["4", "16"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("RD_TAG_LANES", request.param)
    return int(request.param)


def test_the_case_table(lanes):
    groups = {}
    for case in UF.CASES:
        groups.setdefault(tuple(case[2]), []).append(case)
    for names, members in groups.items():
        want, raw_start, _ = _check([_rec(UF.header(c[1], k)[1:], 3 + k % 5, k) for k, c in enumerate(members)], list(names))
        for k, c in enumerate(members):
            assert want[raw_start[k]:raw_start[k + 1]].endswith(UF.expected(c)[0]), c[0]       # what the table says by hand
    _, _, tc = _check([_rec(UF.header(c[1], k)[1:], k % 7, k) for k, c in enumerate(UF.CASES)], NAMES)
    assert tc["malformed_records"] >= 20 and tc["float_values_skipped"] >= 6


def _element_texts(seed, n):
    """n element texts of 1 to 24 bytes, all of them good values"""
    rnd = random.Random(seed)
    pool = [t for _, _, _, t in C.random_texts(seed, 3 * n)] + [b"7", b"0", b"-1", b".5", b"nan", b"-inf", b"1e5", b"12.5"]
    pool = [t for t in pool if len(t) <= 24]
    return [rnd.choice(pool) for _ in range(n)]


def test_f_values_on_every_comment_residue(lanes):
    records, at = [], set()
    values = _element_texts(31, 200)
    for c in range(200):
        name = b"n" * (1 + c % 23)
        head = name + (b"\t" if c % 2 else b" ") + (b"RG:Z:" + b"x" * (c % 7) + b"\t" if c % 3 else b"") + b"qs:f:" + values[c] + (b"\tNM:i:%d" % c if c % 4 == 0 else b"")
        records.append(_rec(head, c % 16, c))
    want, raw_start, tc = _check(records, NAMES)
    assert tc["copied"][0] == 200 and tc["malformed_records"] == 0
    text = U._chunk(records)[0]
    p = 0
    while True:
        p = text.find(b"qs:f:", p + 1)
        if p < 0:
            break
        at.add((p + 5) % 16)
    assert at == set(range(16)), "the values start on every residue modulo 16 of the text"
    tag_at = {(int(raw_start[k + 1]) - len(bam.tags_from_comment(b"@" + r[0], NAMES, True)[0])) % 4 for k, r in enumerate(records)}
    assert tag_at == set(range(4)), "the 4 bytes of a value go to every alignment"


def test_bf_arrays_around_the_lane_count(lanes):
    records = []
    for count in (0, 1, lanes - 1, lanes, lanes + 1, 16 * lanes + 1, 3000):
        for seed in (1, 2):
            els = _element_texts(40 + count + seed, count)
            records.append(_rec(b"a%d.%d\tRG:Z:front\tXF:B:f" % (count, seed) + b"".join(b"," + e for e in els) + b"\tNM:i:%d" % count, count % 9, count))
    lens = {len(e) for e in _element_texts(40 + 3000 + 1, 3000)}
    assert min(lens) == 1 and max(lens) == 24
    records.append(_rec(b"mm\tMM:Z:C+m?" + b",1" * 500 + b";\tXF:B:f" + b",0.25" * 2000 + b"\tML:B:C" + b",255" * 2000, 50))
    want, raw_start, tc = _check(records, NAMES + [b"MM"])
    assert tc["copied"][1] == len(records) and tc["malformed_records"] == 0 and tc["float_values_skipped"] == 0
    off, size, ty = bam.find_tag(want, int(raw_start[13]), b"XF")
    assert ty == ord("B") and size == 5 + 4 * 3000 and struct.unpack_from("<I", want, off + 1)[0] == 3000


@pytest.mark.parametrize("special,malformed", [(LONG, False), (b"1e", True), (b"", True), (b"5.", True)], ids=["skipped", "1e", "empty", "5."])
def test_one_special_element_at_every_place(lanes, special, malformed):
    """an array of 40 elements of 5 text bytes with ONE element that is skipped or malformed, at every place: first, last, and with its
    comma on every byte of a 16-byte piece, so that it also runs across the pieces and the lanes' strides"""
    records = []
    for j in range(40):
        els = [b"12.%d" % (k % 10) for k in range(40)]
        els[j] = special
        records.append(_rec(b"s%d\tRG:Z:a\tXF:B:f" % j + b"".join(b"," + e for e in els) + b"\tNM:i:1", 5, j))
    records.append(_rec(b"good\tRG:Z:a\tXF:B:f" + b",12.5" * 40 + b"\tNM:i:1", 5))
    _, _, tc = _check(records, NAMES)
    assert tc["malformed_records"] == (40 if malformed else 0) and tc["float_values_skipped"] == (0 if malformed else 40)
    assert tc["copied"][1] == 1 and tc["copied"][2] == (1 if malformed else 41)


def _float_field(rnd):
    name = rnd.choice((b"qs", b"XF", b"XX"))
    kind = rnd.randrange(10)
    good = [t for _, _, _, t in C.random_texts(rnd.randrange(1 << 30), 4)]
    if kind < 4:
        return name + b":f:" + good[0]
    if kind < 7:
        return name + b":B:f" + b"".join(b"," + g for g in good[:rnd.randrange(0, 5)] * rnd.choice((1, 1, 9)))
    if kind == 7:
        return rnd.choice((name + b":f:" + LONG, name + b":B:f,1," + LONG + b",2", name + b":B:f," + LONG))
    return rnd.choice((name + b":f:", name + b":f:1e", name + b":f:0x1p3", name + b":B:f,", name + b":B:f,1,,2", name + b":B:f1", name + b":B:f,1,x", name + b":f:nan(1)"))


def _sweep(n, seed, floats=True):
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        fields = []
        for _ in range(rnd.randrange(0, 5)):
            f = _float_field(rnd) if floats and rnd.random() < 0.5 else UT.random_field(rnd)
            if not floats and (f[3:5] == b"f:" or f[3:6] == b"B:f"):
                continue
            fields.append(f)
        sep = (b" ", b"\t", b"\t", b"")[k % 4]
        head = b"r%d" % k + (sep + b"\t".join(fields) if sep else b"") + (b"\r" if k % 97 == 0 else b"")
        ls = rnd.randrange(0, 60)
        out.append((head, bytes(rnd.choice(b"ACGTN") for _ in range(ls)), bytes(rnd.randrange(33, 75) for _ in range(ls))))
    return out


def test_sweep_of_2000_records(lanes):
    _, _, tc = _check(_sweep(2000, 33), [b"qs", b"XF", b"RG", b"ML", b"XI", b"MM"])
    assert min(tc["copied"][:3]) > 50 and tc["malformed_records"] > 100 and tc["float_values_skipped"] > 20


def test_without_f_fields_the_bit_changes_nothing(lanes):
    from ribodetector_amd import ubam
    records = _sweep(2000, 34, floats=False)
    text, rs, so, sl = U._chunk(records)
    names = [b"MM", b"ML", b"RG", b"XI"]
    assert b":f:" not in text and b":B:f" not in text and bam.ubam_tag_counts(text, names)["copied"][2] > 100
    a = _encode(text, rs, so, sl, len(records), ubam.flags_word(), names, floats=False)
    b = _encode(text, rs, so, sl, len(records), ubam.flags_word(), names, floats=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[0][:int(a[2][1])].tobytes() == bam.from_fastq(text, tags=names)


def test_the_bit_needs_names():
    import torch
    from ribodetector_amd import ubam
    records = [_rec(b"r%d\tqs:f:1.5" % k, 8, k) for k in range(10)]
    text, rs, so, sl = U._chunk(records)
    n, lib = len(records), N.lib()
    cap = bam.ubam_bound(len(text), n)
    raw = torch.full((cap + 256,), U.FILL, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV)
    tabs = [torch.from_numpy(x).to(DEV) for x in (rs, so, sl)]
    raw_start = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    info = torch.zeros(12, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(lib.rd_bam_encode_tags_workspace_bytes(n, 1)), dtype=torch.uint8, device=DEV)
    flags = ubam.flags_word() | N.UBAM_TAG_FLOATS
    assert N.UBAM_TAG_FLOATS == 1 << 28
    head = (N.ptr(t), len(text), *(N.ptr(x) for x in tabs), n, 0, 1, flags)
    tail = (N.ptr(raw), cap, N.ptr(raw_start), N.ptr(info), N.ptr(ws), ws.numel(), None)
    assert lib.rd_bam_encode_ex(*head, None, 0, *tail) == -1 and b"RD_UBAM_TAG_FLOATS" in lib.rd_last_error()
    assert lib.rd_bam_encode(*head, *tail) == -1 and b"RD_UBAM_TAG_FLOATS" in lib.rd_last_error()
    assert lib.rd_bam_encode_ex(*head[:-1], flags | (1 << 29), b"qs", 1, *tail) == -1, "the bits above stay unknown"
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == U.FILL).all()
    assert lib.rd_bam_encode_ex(*head, b"qs", 1, *tail) == 0
    torch.cuda.synchronize()
    assert info.cpu().numpy()[:11].tolist() == [n, len(bam.from_fastq(text, tags=[b"qs"], floats=True)), -1, 0, 0, 0, 0, -1, 0, 0, n]
    with pytest.raises(ValueError, match="needs tags"):
        ubam.encode(t, *tabs, n, ubam.flags_word(), floats=True)


def test_raw_cap_one_byte_short():
    from ribodetector_amd import ubam
    records = _sweep(1500, 35)
    names = [b"qs", b"XF", b"RG", b"ML"]
    text, rs, so, sl = U._chunk(records)
    want = bam.from_fastq(text, tags=names, floats=True)
    assert len(want) != len(bam.from_fastq(text, tags=names))
    got, raw_start, info = _encode(text, rs, so, sl, len(records), ubam.flags_word(), names, raw_cap=len(want) - 1)
    assert info[3] == 1 and info[0] == 0 and info[1] == len(want), "fault 1 and the exact need"
    assert (got == U.FILL).all() and (raw_start == 0).all()
    _check(records, names, raw_cap=int(info[1]))


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
LIST = "qs,rq,ML,RG,XF"
CLI_NAMES = [b"qs", b"rq", b"ML", b"RG", b"XF"]


def _comment(i, rng):
    qs = b"\tqs:f:%.4f" % (5.0 + (i * 37 % 35000) / 1000.0)
    full = qs + b"\trq:f:%s" % C.g_text(F.bits_of(0.9 + (i % 100) / 1001.0)) + b"\tML:B:C" + b"".join(b",%d" % v for v in rng.integers(0, 256, i % 9)) + \
        b"\tRG:Z:lib%d" % (i % 3) + b"\tXF:B:f" + b"".join(b",%s" % C.g_text(int(b)) for b in rng.integers(0, 1 << 32, i % 6, dtype=np.uint64))
    return (full, full, full, qs, b" 1:N:0:ACGT", b"", b"\tqs:f:" + LONG + b"\tRG:Z:lib1", b"\tqs:f:1e\tRG:Z:lib2", b"\tXF:B:f,1,,2", full)[i % 10]


@pytest.fixture(scope="module")
def fastq_input(tmp_path_factory):
    from ribodetector_amd import synth
    path = str(tmp_path_factory.mktemp("ubamfloats") / "se.fq")
    a, o, _ = synth.reads_numpy(400, (60, 120), seed=61, rrna_frac=0.3)
    raw, rng = a.tobytes(), np.random.default_rng(61)
    with open(path, "wb") as fh:
        for i in range(len(o) - 1):
            s = raw[o[i]:o[i + 1]]
            fh.write(b"@syn.%d" % i + _comment(i, rng) + b"\n" + s + b"\n+\n" + bytes(rng.integers(33, 75, len(s), dtype=np.uint8)) + b"\n")
    return path


def _cli(tmp_path, caplog, src, floats):
    d = tmp_path / ("floats" if floats else "plain")
    d.mkdir()
    o, r, summ = str(d / "o.bam"), str(d / "r.bam"), str(d / "summary.json")
    caplog.clear()
    with caplog.at_level(logging.INFO):
        p = U._run(["-l", "100", "-i", src, "-o", o, "-r", r, "--summary", summ, "--ubam_output", "--ubam_tags", LIST] + (["--ubam_tag_floats"] if floats else []) + U.SMALL)
    return p, (o, r), open(summ, "rb").read(), caplog.text


def test_cli_single_end_with_and_without_the_flag(tmp_path, fastq_input, caplog):
    from ribodetector_amd import ubam
    text = U._read(fastq_input)
    recs = {x.split(b"\n")[0].split()[0][1:]: x for x in (b"\n".join(q) + b"\n" for q in zip(*[iter(text.split(b"\n")[:-1])] * 4))}
    docs = {}
    for floats in (True, False):
        p, outs, raw, log = _cli(tmp_path, caplog, fastq_input, floats)
        assert p.num_read == 400
        kw = {"floats": True} if floats else {}            # (without the flag: the calls as they were before the keyword existed)
        tagged = 0
        for path in outs:
            data = U._inflate_bam(path)
            mine = b"".join(recs[x.name] for x in bam.records(data))
            assert data == U.HEADER + bam.from_fastq(mine, tags=CLI_NAMES, **kw), path
            tagged += len(data)
        tc = bam.ubam_tag_counts(text, CLI_NAMES, **kw)
        doc = json.loads(raw)
        assert doc["ubam_tags"] == ubam.to_json_tags(CLI_NAMES, [tc], **kw)
        assert ubam.log_line_tags(CLI_NAMES, [tc]) in log and "BAM tags from text: qs " in log
        assert (list(doc["ubam_tags"])[-1] == "float_rounding") == floats and list(doc)[-1] == "ubam_tags"
        docs[floats] = (doc, raw, tagged, tc)
    on, off = docs[True][3], docs[False][3]
    assert on["copied"][0] == 200 and off["copied"][0] == 0 and on["float_values_skipped"] == 40 and off["float_values_skipped"] > 600
    assert on["malformed_records"] == 80 and off["malformed_records"] == 0 and docs[True][2] > docs[False][2]
    assert list(docs[True][0]) == list(docs[False][0]) and b"float_rounding" not in docs[False][1]
    assert list(docs[True][0]["ubam_tags"])[:-1] == list(docs[False][0]["ubam_tags"])


def test_cli_round_trip_bam_fastq_bam_fastq(tmp_path):
    """BAM with qs:f, rq:f, ML:B:C, RG:Z and a B:f -> --bam_tags --bam_tag_floats -> --ubam_output --ubam_tags --ubam_tag_floats ->
    --bam_tags --bam_tag_floats: the two FASTQ texts hold the same records (guarantee (a), through the device both ways)"""
    hard = F.hard()
    recs = []
    for i in range(300):
        tags = F.f_tag(b"qs", F.bits_of(5.0 + (i * 37 % 3500) / 100.0) if i % 8 else hard[(i * 13) % 4000]) + F.f_tag(b"rq", hard[(i * 7 + 1) % 4000])
        tags += BT.B(b"ML", "C", [(i * k) % 256 for k in range(i % 12)]) + BT.Z(b"RG", b"grp%d" % (i % 3)) + F.bf_tag(b"XF", hard[i:i + i % 7] + F.NANS[:i % 3])
        seq = "".join("ACGT"[(i * 7 + j * j + j // 3) % 4] for j in range(60 + i % 41))
        recs.append(BT.rec(tags, name=b"read%d" % i, seq=seq, flag=4))
    src = str(tmp_path / "in.bam")
    bam.write_bam(src, recs)

    def to_fastq(paths, tag):
        out = []
        for k, path in enumerate(paths):
            o, r = str(tmp_path / ("%s%d.o.fq" % (tag, k))), str(tmp_path / ("%s%d.r.fq" % (tag, k)))
            U._run(["-l", "100", "-i", path, "-o", o, "-r", r, "--bam_tags", LIST, "--bam_tag_floats"] + U.SMALL)
            out += [o, r]
        return out

    first = to_fastq([src], "a")
    bams = []
    for k, fq in enumerate(first):
        o, r = str(tmp_path / ("b%d.o.bam" % k)), str(tmp_path / ("b%d.r.bam" % k))
        U._run(["-l", "100", "-i", fq, "-o", o, "-r", r, "--ubam_output", "--ubam_tags", LIST, "--ubam_tag_floats"] + U.SMALL)
        bams += [o, r]
    second = to_fastq(bams, "c")
    quads = lambda paths: sorted(b"\n".join(q) for p in paths for q in zip(*[iter(U._read(p).split(b"\n")[:-1])] * 4))      # noqa: E731
    a, c = quads(first), quads(second)
    assert len(a) == 300 and a == c
    assert sum(q.count(b":f:") for q in a) == 600 and sum(b"XF:B:f" in q for q in a) == 300 and any(b"nan" in q for q in a)
    data = b"".join(U._inflate_bam(p)[len(U.HEADER):] for p in bams)
    assert sorted(data) != [] and len(list(bam.records(U.HEADER + data))) == 300
