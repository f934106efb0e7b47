"""--interleaved on the GPU: rd_pair_split / rd_pair_expand_labels against the pure-Python reference of tests/test_interleaved_host.py,
and the CLI on one interleaved file against the CLI on the same pairs as two files (and, once, against the oracle)."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_interleaved_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["none", "rrna", "norrna", "both"]


def _read(path):
    if not os.path.exists(path):
        return None
    with (gzip.open if path.endswith("gz") else open)(path, "rb") as fh:
        return fh.read()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _split(records, n_pairs=None, check_ids=True, tables=None):
    """rd_pair_split over the records' tables -> (pair_start, off1, len1, off2, len2 as lists, info as a list)"""
    import torch
    from ribodetector_amd.gz import DevicePairSplit
    text, rs, so, sl = tables if tables is not None else H.tables_of(records)
    n = (len(rs) - 1) // 2 if n_pairs is None else n_pairs
    t = _dev(np.frombuffer(text + b"\0", np.uint8))[:len(text)]
    ps, m1, m2, info = DevicePairSplit("cuda:0").split(t, _dev(rs), _dev(so), _dev(sl), n, check_ids=check_ids)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (ps, m1[0], m1[1], m2[0], m2[1])], [int(v) for v in info.cpu()]


def _check_split(records, check_ids=True):
    got, info = _split(records, check_ids=check_ids)
    _, rs, so, sl = H.tables_of(records)
    want = H.split_tables(rs, so, sl)
    for g, w, dt in zip(got, want, (np.int64, np.int64, np.int32, np.int64, np.int32)):
        assert g.dtype == dt and np.array_equal(g, np.asarray(w, dtype=dt))         # bit-exact
    return info


@pytest.mark.parametrize("n", [0, 1, 7, (1 << 17) + 3])
def test_pair_split_against_the_reference(n):
    r1, r2 = H.synth_pairs(n, seed=100 + n % 97)
    recs = H.interleave(r1, r2)
    assert _check_split(recs) == [n, -1, 0, 0]
    assert _check_split(recs, check_ids=False) == [n, -1, 0, 0]
    if n == 0:
        return
    rng = np.random.default_rng(n)
    ks = sorted(int(k) for k in rng.choice(n, size=min(2, n), replace=False))
    other = lambda k: b"@someone_else_%d/2 x\nAC\n+\nII\n" % k      # noqa: E731
    one = list(recs)
    one[2 * ks[-1] + 1] = other(ks[-1])                     # a mismatch planted at a random pair
    assert H.first_mismatch(one) == ks[-1] and _check_split(one) == [n, ks[-1], 0, 0]
    assert _check_split(one, check_ids=False) == [n, -1, 0, 0]
    if len(ks) == 2:                                        # two mismatches (they need two pairs): the first one wins
        two = list(one)
        two[2 * ks[0]] = other(ks[0])
        assert H.first_mismatch(two) == ks[0] and _check_split(two) == [n, ks[0], 0, 0]
        assert _check_split(two, check_ids=False) == [n, -1, 0, 0]
    last = list(recs)
    last[-1] = other(n)                                     # the first mismatch in the last pair
    assert _check_split(last) == [n, n - 1, 0, 0]


def test_pair_split_hand_built_ids():
    rec = lambda h: h + b"\nACGT\n+\nIIII\n"      # noqa: E731
    cases = [(b"@r1", b"@r1", True), (b"@r1/1", b"@r1/2", True), (b"@r1/2", b"@r1/1", False), (b"@r1/1", b"@r1/1", True), (b"@r1 1:N", b"@r1 2:N", True),
             (b"@", b"@ c", True), (b"@r1\r", b"@r1\r", True), (b"@r1", b"@r11", False), (b"@/1", b"@/2", True), (b"@1", b"@2", False),
             (b"@" + b"a" * 15 + b"/1", b"@" + b"a" * 15 + b"/2", True), (b"@" + b"a" * 16 + b"/1", b"@" + b"a" * 16 + b"/2", True),
             (b"@" + b"a" * 17, b"@" + b"a" * 16 + b"b", False), (b"@" + b"a" * 40 + b"/1", b"@" + b"a" * 39 + b"b/2", False),
             (b"@" + b"a" * 33, b"@" + b"a" * 33 + b" y", True), (b"@b" + b"a" * 32, b"@c" + b"a" * 32, False)]
    for h1, h2, mates in cases:
        assert H.are_mates(H.read_id(rec(h1)), H.read_id(rec(h2))) is mates
        assert _check_split([rec(b"@p"), rec(b"@p"), rec(h1), rec(h2)]) == [2, -1 if mates else 1, 0, 0], (h1, h2)


def test_pair_split_faults_are_reported_not_followed():
    r1, r2 = H.synth_pairs(300, seed=8)
    recs = H.interleave(r1, r2)
    text, rs, so, sl = H.tables_of(recs)
    for what in ("rec_start", "seq_off", "order"):
        rs2, so2 = rs.copy(), so.copy()
        if what == "rec_start":
            rs2[-1] = len(text) + 5                         # a table entry outside the text
        elif what == "seq_off":
            so2[17] = len(text)
        else:
            rs2[100] = rs2[101]
        _, info = _split(None, tables=(text, rs2, so2, sl))
        assert info[3] != 0, what
    bad = list(recs)
    bad[41] = b"+not a header\nAC\n+\nII\n"                   # a record that does not start with '@'
    assert _split(bad)[1][3] != 0 and _split(bad, check_ids=False)[1] == [300, -1, 0, 0]
    text, rs, so, sl = H.tables_of(recs[:3])
    text += b"@header_without_an_end"                       # the header line runs past the record
    tables = (text, np.append(rs, len(text)), np.append(so, len(text)), np.append(sl, 0).astype(np.int32))
    assert _split(None, tables=tables)[1][3] != 0 and _split(None, tables=tables, check_ids=False)[1] == [2, -1, 0, 0]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 2049, (1 << 17) + 3])
def test_pair_expand_labels(n):
    import torch
    from ribodetector_amd import _native as N
    from ribodetector_amd.gz import DevicePairSplit
    assert N.LABEL_SKIP == H.LABEL_SKIP
    labels = np.random.default_rng(n).integers(-1, 2, n).astype(np.int8)
    d = DevicePairSplit("cuda:0")
    for mate in (0, 1):
        got = d.expand(_dev(labels), mate)
        torch.cuda.synchronize()
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), np.asarray(H.expand_labels(labels, mate), dtype=np.int8))


def test_split_outputs_are_the_existing_selection_over_expanded_labels():
    """the records of ONE mate by label = rd_select_pack / rd_gz_compress_selected over the full record table with rd_pair_expand_labels'
    labels; the pairs by label = the same two over pair_start with the pair labels"""
    import torch
    from ribodetector_amd.gz import DeviceGzip, DevicePairSplit, DeviceSelect
    n = 5000
    r1, r2 = H.synth_pairs(n, seed=12)
    recs = H.interleave(r1, r2)
    text, rs, so, sl = H.tables_of(recs)
    t = _dev(np.frombuffer(text, np.uint8))
    labels = np.random.default_rng(3).integers(-1, 2, n).astype(np.int8)
    d, sel, gz = DevicePairSplit("cuda:0"), DeviceSelect("cuda:0"), DeviceGzip("cuda:0")
    ps, _, _, _ = d.split(t, _dev(rs), _dev(so), _dev(sl), n)
    for want in (0, 1, -1):
        out, info = sel.pack_selected(t, ps, _dev(labels), want)
        torch.cuda.synchronize()
        assert int(info[3]) == 0 and out[:int(info[1])].cpu().numpy().tobytes() == b"".join(H.interleave(
            [r for r, lab in zip(r1, labels) if lab == want], [r for r, lab in zip(r2, labels) if lab == want]))
        for mate, mine in enumerate((r1, r2)):
            e = d.expand(_dev(labels), mate)
            out, info = sel.pack_selected(t, _dev(rs), e, want)
            torch.cuda.synchronize()
            assert int(info[3]) == 0 and out[:int(info[1])].cpu().numpy().tobytes() == H.select(mine, labels, want)
            out, info = gz.compress_selected(t, _dev(rs), e, want)
            torch.cuda.synchronize()
            assert gzip.decompress(out[:int(info[0])].cpu().numpy().tobytes()) == H.select(mine, labels, want)


# ---- the CLI against the two-file run ------------------------------------------------------------------------------------------------
def _records(arena, off, mate):
    b = arena.tobytes()
    out = []
    for i in range(len(off) - 1):
        s = b[off[i]:off[i + 1]]
        out.append(b"@syn.%d/%d\n%s\n+\n%s\n" % (i, mate, s, b"I" * len(s)))
    return out


def _run(args, env=None):
    """detect.main in this process with environment variables set for the call"""
    from ribodetector_amd import detect
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        p = detect.main(args)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return p


def _counters(p):
    return (p.num_read, p.num_nonrrna, p.num_rrna, p.num_unknown)


SMALL = ["--chunk_size", "1", "-m", "3"]      # chunks of CHUNK pairs at -l 100: several chunks and a short last one for 3,000 pairs
CHUNK = 512


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """the pairs of test_gpu_cli.test_cli_paired (3,000 pairs, 60-120 bp, seeds 41 / 42; ids end /1 and /2) as two files and as one
    interleaved file (plain, and one gzip stream of zlib level 6), and the two-file run's outputs for every -e mode"""
    from ribodetector_amd import synth
    d = tmp_path_factory.mktemp("pairs")
    n = 3000
    a1, o1, l1 = synth.reads_numpy(n, (60, 120), seed=41, rrna_frac=0.3)
    a2, o2, l2 = synth.reads_numpy(n, (60, 120), seed=42, rrna_frac=0.3)
    i1, i2 = str(d / "r_1.fq"), str(d / "r_2.fq")
    synth.write_fastq(i1, a1, o1, 1)
    synth.write_fastq(i2, a2, o2, 2)
    r1, r2 = _records(a1, o1, 1), _records(a2, o2, 2)
    assert open(i1, "rb").read() == b"".join(r1) and open(i2, "rb").read() == b"".join(r2)
    il = str(d / "il.fq")
    open(il, "wb").write(b"".join(H.interleave(r1, r2)))
    open(il + ".gz", "wb").write(gzip.compress(open(il, "rb").read(), 6))
    two = {}
    for e in MODES:
        f = {k: str(d / ("two_%s_%s" % (e, k))) for k in ("o1.fq", "o2.fq", "r1.fq", "r2.fq", "rep.tsv")}
        p = _run(["-l", "100", "-i", i1, i2, "-o", f["o1.fq"], f["o2.fq"], "-r", f["r1.fq"], f["r2.fq"], "-e", e, "--read_report", f["rep.tsv"]] + SMALL)
        two[e] = {"files": {k: _read(v) for k, v in f.items()}, "counters": _counters(p)}
        two[e]["files"]["u1"], two[e]["files"]["u2"] = _read(f["o1.fq"] + ".unclassified.gz"), _read(f["o2.fq"] + ".unclassified.gz")
        assert p.num_read == n and (two[e]["files"]["u1"] is not None) == (e == "both")
    return {"n": n, "dir": d, "i": (i1, i2), "il": il, "r": (r1, r2), "arrays": ((a1, o1, l1), (a2, o2, l2)), "two": two}


def _fastq_records(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def _interleave_blobs(b1, b2):
    if b1 is None:
        assert b2 is None
        return None
    return b"".join(H.interleave(_fastq_records(b1), _fastq_records(b2)))


def _check_against_two(tmp, pairs, ensure, inp, out_kind, gz_out, env=None, tag="x", extra=()):
    """one interleaved run; its files against the two-file run's"""
    two = pairs["two"][ensure]
    ext = ".fq.gz" if gz_out else ".fq"
    rep = str(tmp / ("%s_rep.tsv%s" % (tag, ".gz" if gz_out else "")))
    if out_kind == "interleaved":
        o, r = [str(tmp / (tag + "_o" + ext))], [str(tmp / (tag + "_r" + ext))]
    else:
        o, r = [str(tmp / (tag + "_o%d" % e + ext)) for e in (1, 2)], [str(tmp / (tag + "_r%d" % e + ext)) for e in (1, 2)]
    p = _run(["-l", "100", "-i", inp, "--interleaved", "-o", *o, "-r", *r, "-e", ensure, "--read_report", rep] + list(extra) + SMALL, env)
    assert _counters(p) == two["counters"]
    f = two["files"]
    if out_kind == "interleaved":
        assert _read(o[0]) == _interleave_blobs(f["o1.fq"], f["o2.fq"]) and _read(r[0]) == _interleave_blobs(f["r1.fq"], f["r2.fq"])
        assert _read(o[0] + ".unclassified.gz") == _interleave_blobs(f["u1"], f["u2"])
    else:
        assert [_read(x) for x in o + r] == [f["o1.fq"], f["o2.fq"], f["r1.fq"], f["r2.fq"]]
        assert [_read(x + ".unclassified.gz") for x in o] == [f["u1"], f["u2"]]
    assert _read(rep) == f["rep.tsv"] and f["rep.tsv"].startswith(b"#read_id\tlabel\tp_rrna_1\tp_rrna_2\tp_rrna_pair\nsyn.")
    if gz_out and shutil.which("gzip"):
        for x in o + r + [rep]:
            assert subprocess.run(["gzip", "-t", x], capture_output=True, timeout=120).returncode == 0
    return p, o, r


@pytest.mark.parametrize("ensure", MODES)
@pytest.mark.parametrize("out_kind", ["interleaved", "split"])
def test_cli_interleaved_matches_two_files(tmp_path, pairs, ensure, out_kind):
    p, _, _ = _check_against_two(tmp_path, pairs, ensure, pairs["il"], out_kind, False)
    assert p.is_paired and p.ingest["il.fq"]["path"] == "device"
    assert len(pairs["two"][ensure]["files"]["o1.fq"]) > 0 and len(pairs["two"][ensure]["files"]["r1.fq"]) > 0


def test_cli_interleaved_stands_on_the_oracle(tmp_path, pairs, oracle):
    """the labels of the interleaved run against oracle.pair_fuse, with the margin assertion of test_gpu_cli.test_cli_paired"""
    (a1, o1, l1), (a2, o2, l2) = pairs["arrays"]
    r1, r2 = pairs["r"]
    g1, g2 = oracle.forward_packed(a1, o1, l1, 100), oracle.forward_packed(a2, o2, l2, 100)
    m1, m2 = np.abs(g1[:, 1] - g1[:, 0]), np.abs(g2[:, 1] - g2[:, 0])
    ms = np.abs((g1[:, 1] + g2[:, 1]) - (g1[:, 0] + g2[:, 0]))
    assert min(m1.min(), m2.min(), ms.min()) > 2e-4
    for ensure in ("none", "both"):
        lab = oracle.pair_fuse(g1, g2, ensure)
        o, r = str(tmp_path / ("o_%s.fq" % ensure)), str(tmp_path / ("r_%s.fq" % ensure))
        p = _run(["-l", "100", "-i", pairs["il"], "--interleaved", "-o", o, "-r", r, "-e", ensure] + SMALL)
        assert p.num_read == pairs["n"] and p.num_nonrrna == int((lab == 0).sum()) and p.num_rrna == int((lab == 1).sum())
        for path, want in ((o, 0), (r, 1)) + (((o + ".unclassified.gz", -1),) if ensure == "both" else ()):
            idx = np.flatnonzero(lab == want)
            assert _read(path) == b"".join(H.interleave([r1[i] for i in idx], [r2[i] for i in idx]))
        if ensure == "both":
            assert p.num_unknown == int((lab == -1).sum()) > 0


@pytest.mark.parametrize("kind", ["gz", "bgzf", "host", "host-gz"])
@pytest.mark.parametrize("out_kind,gz_out", [("interleaved", False), ("interleaved", True), ("split", False), ("split", True)])
def test_cli_interleaved_input_and_output_kinds(tmp_path, pairs, kind, out_kind, gz_out):
    """single-stream .gz (zlib 6), BGZF (a .gz written by this CLI), RD_INGEST=host (plain and .gz); plain outputs and .gz outputs
    deflated on the device"""
    env, inp, data = None, pairs["il"] + ".gz", pairs
    if kind == "bgzf":
        # the CLI's own interleaved .gz output (the non-rRNA pairs of -e none) is the input; the two-file run it is held to reads the
        # same pairs from the two-file run's plain non-rRNA outputs
        d = tmp_path
        src = pairs["two"]["none"]["files"]
        i1, i2 = str(d / "b_1.fq"), str(d / "b_2.fq")
        open(i1, "wb").write(src["o1.fq"])
        open(i2, "wb").write(src["o2.fq"])
        inp = str(d / "bgzf_il.fq.gz")
        _run(["-l", "100", "-i", pairs["il"], "--interleaved", "-o", inp] + SMALL)
        from ribodetector_amd.gz import is_member_indexed
        assert is_member_indexed(inp) == "BC" and _read(inp) == _interleave_blobs(src["o1.fq"], src["o2.fq"])
        f = {k: str(d / ("btwo_" + k)) for k in ("o1.fq", "o2.fq", "r1.fq", "r2.fq", "rep.tsv")}
        p = _run(["-l", "100", "-i", i1, i2, "-o", f["o1.fq"], f["o2.fq"], "-r", f["r1.fq"], f["r2.fq"], "-e", "both", "--read_report", f["rep.tsv"]] + SMALL)
        files = {k: _read(v) for k, v in f.items()}
        files["u1"], files["u2"] = _read(f["o1.fq"] + ".unclassified.gz"), _read(f["o2.fq"] + ".unclassified.gz")
        data = dict(pairs, two={"both": {"files": files, "counters": _counters(p)}})
    elif kind.startswith("host"):
        env, inp = {"RD_INGEST": "host"}, pairs["il"] + (".gz" if kind == "host-gz" else "")
    p, _, _ = _check_against_two(tmp_path, data, "both", inp, out_kind, gz_out, env=env)
    took = p.ingest.get(os.path.basename(inp), {}).get("path")
    assert took != "device" if kind.startswith("host") else took is not None      # (a small .gz stream may be given back to the host's decoders)
    if kind == "bgzf":
        assert took == "device"


def test_cli_interleaved_whole_file_mode(tmp_path):
    """2^17 + 1 pairs without --chunk_size: the first chunk of 2^17 pairs and a last chunk of one pair"""
    from ribodetector_amd import synth
    n = (1 << 17) + 1
    a1, o1, _ = synth.reads_numpy(n, (60, 120), seed=43, rrna_frac=0.3)
    a2, o2, _ = synth.reads_numpy(n, (60, 120), seed=44, rrna_frac=0.3)
    i1, i2, il = str(tmp_path / "w_1.fq"), str(tmp_path / "w_2.fq"), str(tmp_path / "w_il.fq")
    synth.write_fastq(i1, a1, o1, 1)
    synth.write_fastq(i2, a2, o2, 2)
    r1, r2 = _fastq_records(open(i1, "rb").read()), _fastq_records(open(i2, "rb").read())
    open(il, "wb").write(b"".join(H.interleave(r1, r2)))
    t = [str(tmp_path / x) for x in ("t1.fq", "t2.fq", "t.tsv")]
    p2 = _run(["-l", "100", "-i", i1, i2, "-o", t[0], t[1], "--read_report", t[2]])
    s = [str(tmp_path / x) for x in ("s1.fq", "s2.fq", "s.tsv")]
    ps = _run(["-l", "100", "-i", il, "--interleaved", "-o", s[0], s[1], "--read_report", s[2]])
    o = [str(tmp_path / x) for x in ("o.fq", "o.tsv")]
    po = _run(["-l", "100", "-i", il, "--interleaved", "-o", o[0], "--read_report", o[1]])
    assert _counters(p2) == _counters(ps) == _counters(po) and p2.num_read == n
    assert [_read(x) for x in s] == [_read(x) for x in t] and _read(o[1]) == _read(t[2])
    assert _read(o[0]) == _interleave_blobs(_read(t[0]), _read(t[1]))


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_cli_interleaved_argument_errors(tmp_path, pairs):
    from ribodetector_amd import detect
    with pytest.raises(RuntimeError, match="--interleaved"):
        detect.main(["-l", "100", "-i", *pairs["i"], "--interleaved", "-o", str(tmp_path / "x.fq")])
    with pytest.raises(RuntimeError, match="--interleaved"):
        detect.main(["-l", "100", "-i", pairs["il"], "--interleaved", "-o", str(tmp_path / "x.fq"), "-r", str(tmp_path / "a.fq"), str(tmp_path / "b.fq")])
    with pytest.raises(RuntimeError, match="interleaved FASTA is not supported"):
        detect.main(["-l", "100", "-i", str(tmp_path / "x.fa"), "--interleaved", "-o", str(tmp_path / "y.fa")])


@pytest.mark.parametrize("env", [None, {"RD_INGEST": "host"}])
def test_cli_odd_record_count(tmp_path, pairs, env):
    """the pairs in front of the lone record are classified and written, then the error"""
    il = str(tmp_path / "odd.fq")
    open(il, "wb").write(open(pairs["il"], "rb").read() + b"@lonely/1\nACGT\n+\nIIII\n")
    o, r = str(tmp_path / "o.fq"), str(tmp_path / "r.fq")
    with pytest.raises(ValueError) as e:
        _run(["-l", "100", "-i", il, "--interleaved", "-o", o, "-r", r] + SMALL, env)
    assert str(e.value) == "interleaved input holds an odd number of records (%d): the last record has no mate" % (2 * pairs["n"] + 1)
    f = pairs["two"]["none"]["files"]
    assert _read(o) == _interleave_blobs(f["o1.fq"], f["o2.fq"]) and _read(r) == _interleave_blobs(f["r1.fq"], f["r2.fq"])


@pytest.mark.parametrize("env", [None, {"RD_INGEST": "host"}])
def test_cli_deleted_record_fails_the_mate_check(tmp_path, pairs, env):
    """a record deleted in the second chunk (chunks of CHUNK pairs): every later pair is shifted. RuntimeError with both ids and the
    record numbers; the first chunk's pairs are in the output; --no_mate_check runs through"""
    r1, r2 = pairs["r"]
    recs = H.interleave(r1, r2)
    k = 700                                                  # pair 700, in the second chunk: its mate 1 (record 1401, 1-based) goes
    del recs[2 * k]
    recs.append(b"@syn.tail\nACGT\n+\nIIII\n")               # (an even record count again)
    il = str(tmp_path / "del.fq")
    open(il, "wb").write(b"".join(recs))
    o, r = str(tmp_path / "o.fq"), str(tmp_path / "r.fq")
    with pytest.raises(RuntimeError) as e:
        _run(["-l", "100", "-i", il, "--interleaved", "-o", o, "-r", r] + SMALL, env)
    msg = str(e.value)
    assert "records 1401 and 1402" in msg and "'syn.700/2'" in msg and "'syn.701/1'" in msg and "--no_mate_check" in msg
    f = pairs["two"]["none"]["files"]
    want_o, want_r = _interleave_blobs(f["o1.fq"], f["o2.fq"]), _interleave_blobs(f["r1.fq"], f["r2.fq"])
    first = set(H.interleave(r1[:CHUNK], r2[:CHUNK]))        # the first chunk's pairs are written, the failing chunk's are not
    heads = [b"".join(x for x in _fastq_records(want) if x in first) for want in (want_o, want_r)]
    assert [_read(o), _read(r)] == heads and min(len(h) for h in heads) > 0
    p = _run(["-l", "100", "-i", il, "--interleaved", "--no_mate_check", "-o", o, "-r", r] + SMALL, env)
    assert p.num_read == pairs["n"] and _read(o).startswith(heads[0]) and _read(r).startswith(heads[1]) and len(_read(o)) + len(_read(r)) == len(b"".join(recs))


def test_cli_empty_input(tmp_path):
    il = str(tmp_path / "empty.fq")
    open(il, "wb").close()
    o, r, rep = str(tmp_path / "o.fq"), str(tmp_path / "r.fq.gz"), str(tmp_path / "rep.tsv")
    p = _run(["-l", "100", "-i", il, "--interleaved", "-o", o, "-r", r, "--read_report", rep] + SMALL)
    assert _counters(p) == (0, 0, 0, 0) and _read(o) == b"" and _read(r) == b""
    assert _read(rep) == b"#read_id\tlabel\tp_rrna_1\tp_rrna_2\tp_rrna_pair\n"


# ---- two ranks on the one GPU over gloo ----------------------------------------------------------------------------------------------
def _torchrun(world, args, env_extra=None, timeout=600):
    import socket
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RD_DIST_BACKEND="gloo", RD_LOCAL_DEVICE="0", PYTHONPATH=root, **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ribodetector_amd.detect"] + list(args)
    return subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=timeout), port


@pytest.mark.parametrize("shared", ["1", "0"])
def test_cli_interleaved_two_ranks_match_one(tmp_path, pairs, shared):
    """interleaved .gz -> interleaved .gz plus the report under two ranks: the files of one rank, after decompression; the run takes
    the label-gather layout (one decode into shared memory, or every rank decodes for itself)"""
    inp = pairs["il"] + ".gz"
    one = [str(tmp_path / x) for x in ("a_o.fq.gz", "a_r.fq.gz", "a_rep.tsv.gz")]
    p = _run(["-l", "100", "-i", inp, "--interleaved", "-o", one[0], "-r", one[1], "-e", "both", "--read_report", one[2]] + SMALL)
    two = [str(tmp_path / x) for x in ("b_o.fq.gz", "b_r.fq.gz", "b_rep.tsv.gz")]
    r, port = _torchrun(2, ["-l", "100", "-i", inp, "--interleaved", "-o", two[0], "-r", two[1], "-e", "both", "--read_report", two[2]] + SMALL,
                        {"RD_SHARED_DECODE": shared})
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-3000:]
    assert "label-gather layout" in text and "parses" not in text
    assert p.num_read == pairs["n"] and "Processed" in text and str(pairs["n"]) in text
    for a, b in zip(one + [one[0] + ".unclassified.gz"], two + [two[0] + ".unclassified.gz"]):
        assert _read(a) == _read(b) and len(_read(a)) > 0
    f = pairs["two"]["both"]["files"]
    assert _read(two[0]) == _interleave_blobs(f["o1.fq"], f["o2.fq"]) and _read(two[2]) == f["rep.tsv"]
    assert not [x for x in os.listdir("/dev/shm") if x.startswith("rd_%d_" % port)]
    assert not [x for x in os.listdir(tmp_path) if ".part" in x]
