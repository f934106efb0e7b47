"""Outputs per read group, the parts that need no GPU: the file names of a family (bam.split_name / split_paths / esc), the plain
statement tests/group_truth.py held to itself, and the argument errors of the device calls that return before any HIP call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_truth as GT  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

KEEP = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789._+=@,-"


def test_esc_every_byte():
    for b in range(256):
        got = bam.esc(bytes([b]))
        assert got == (chr(b) if b in KEEP else "%%%02X" % b)
    assert bam.esc(b"a/b %") == "a%2Fb%20%25" and bam.esc(b"") == "" and bam.esc(b"\xff\x00") == "%FF%00"
    assert all("/" not in bam.esc(bytes([b, 47, b])) for b in range(256))


def test_esc_is_injective_over_a_seeded_set():
    rng = np.random.default_rng(1)
    ids = {bytes(rng.choice(list(b"%/ 2F5a.\xe9"), int(rng.integers(1, 7))).astype(np.uint8)) for _ in range(5000)}
    ids |= {b"%", b"%25", b"%2525", b"/", b"%2F", b"unassigned", b"rg-x"}
    assert len({bam.esc(i) for i in ids}) == len(ids)
    names = bam.split_paths("out/non.fq.gz", sorted(ids))
    assert len(set(names)) == len(ids) + 1 and names[-1] == "out/non.unassigned.fq.gz"


def test_split_name_places_the_marker():
    assert bam.split_name("non.fq.gz", b"lib7") == "non.rg-lib7.fq.gz"
    assert bam.split_name("non.fq.gz", None) == "non.unassigned.fq.gz"
    assert bam.split_name("a.b/non", b"x") == "a.b/non.rg-x"                 # no dot in the basename: appended (the directory's dot is not one)
    assert bam.split_name("a.b/non", None) == "a.b/non.unassigned"
    assert bam.split_name(".hidden", b"x") == ".hidden.rg-x"                 # a leading dot is the name's first byte
    assert bam.split_name(".hidden.fq", b"x") == ".hidden.rg-x.fq"
    assert bam.split_name("/abs/dir/r.bam", b"a b") == "/abs/dir/r.rg-a%20b.bam"
    assert bam.split_name("non.fq", b"unassigned") == "non.rg-unassigned.fq" != bam.split_name("non.fq", None)
    long = "n" * 250 + ".fq.gz"                                             # a basename of 256 bytes: the rule itself sets no limit
    assert len(long) == 256 and bam.split_name(long, b"g") == "n" * 250 + ".rg-g.fq.gz"
    assert bam.split_paths("o.fq", [b"b", b"a"]) == ["o.rg-b.fq", "o.rg-a.fq", "o.unassigned.fq"]


def test_unclassified_path_composition():
    from ribodetector_amd.detect import unclassified_path
    for out, raw in (("d/non.fq.gz", False), ("d/non.bam", True), ("non", False)):
        u = unclassified_path(out, raw)
        fam = bam.split_paths(u, [b"lib/1"])
        assert fam == [bam.split_name(u, b"lib/1"), bam.split_name(u, None)] and os.path.dirname(fam[0]) == os.path.dirname(out)
        assert len(set(fam) | set(bam.split_paths(out, [b"lib/1"]))) == 4


def _bam(rng, n, ids):
    """an inflated BAM file of n reads: declared groups (the last one without reads), no RG, an undeclared value, RG:i, a tag cut
    short, secondary and reverse-strand records"""
    import struct
    reads = []
    for i in range(n):
        L = int(rng.integers(20, 60))
        kind = int(rng.integers(0, 9))
        tags = b"NMi" + struct.pack("<i", i % 7)
        if kind < 4:
            tags += b"RGZ" + ids[kind % (len(ids) - 1)] + b"\0"
        elif kind == 4:
            tags += b"RGZnobody\0"
        elif kind == 5:
            tags += b"RGi" + struct.pack("<i", 5)
        elif kind == 6:
            tags += b"RGZcut"                               # (no NUL: the value runs into the record's end)
        flag = 4 | (0x10 if i % 3 == 0 else 0) | (0x100 if i % 11 == 5 else 0)
        reads.append(dict(name=b"r%d" % i, seq=bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)), qual=bytes(rng.integers(2, 40, L).astype(np.uint8)),
                          flag=flag, tags=tags))
    text = b"@HD\tVN:1.6\n" + b"".join(b"@RG\tID:" + i + b"\n" for i in ids)
    return bam.payload(reads, text=text)


@pytest.mark.parametrize("source", ["fastq", "tagged", "raw"])
def test_the_statement_holds_itself(source):
    """the union of a family, merged in input order, is the unsplit selection; every selected record lands in exactly one member; the
    group without reads gets nothing"""
    rng = np.random.default_rng(3)
    ids = [b"lib7", b"a/b %", b"empty"]
    data = _bam(rng, 400, ids)
    delivered = [r for r in bam.records(data) if not r.skipped]
    n = len(delivered)
    labels = rng.integers(-1, 2, n)
    rows = GT.group_rows(data, ids)
    srt, _ = bam.sorted_ids(ids)
    assert set(rows) == {0, 2, 3, 4, 5} and srt == [b"a/b %", b"empty", b"lib7"]       # (row 1, 'empty', has no read)
    tags = [b"RG", b"NM"]
    for label in (-1, 0, 1):
        fam = GT.split_select(data, labels, ids, label, source, tags)
        keep = [k for k in range(n) if labels[k] == label]
        if source == "raw":
            whole = bam.select(data, keep)
            unit = [data[r.offset:r.offset + r.size] for r in delivered]
        else:
            text = bam.fastq_text_tagged(data, tags) if source == "tagged" else bam.fastq_text(data)
            unit, at = [], 0
            for r in delivered:
                size = len(r.fastq()) + (len(bam.tag_comment(data, r.offset, tags)[0]) if source == "tagged" else 0)
                unit.append(text[at:at + size])
                at += size
            whole = b"".join(unit[k] for k in keep)
        assert len(fam) == len(ids) + 1 and fam[1] == b"" and sum(len(m) for m in fam) == len(whole)
        cursor, merged = [0] * len(fam), []
        for k in keep:                                   # merge in input order: record k must be the next bytes of ITS member, of no other
            g = min(rows[k], len(ids))
            assert fam[g][cursor[g]:cursor[g] + len(unit[k])] == unit[k]
            cursor[g] += len(unit[k])
            merged.append(unit[k])
        assert cursor == [len(m) for m in fam] and b"".join(merged) == whole


def test_keys_and_partition_statement():
    rows, labels = [0, 1, 2, 3, 4, 1], [1, 0, -1, 1, 1, 0]
    assert GT.keys(rows, labels, [-1, 0, 1], 2) == ([3, 1, -1, 5, 5, 1], 0)
    assert GT.keys(rows, labels[:3], [2, 0, 1], 2, 0, 2, 1) == ([-1, 3, -1, 2, -1, 8], 0)
    assert GT.keys([0, 9], [1, 5], [0, 1, 2], 2) == ([6, -1], 3)
    text, rs = b"aabcccd", [0, 2, 3, 6, 6, 7]
    runs = GT.partition(text, rs, [1, 0, 1, 1, -1], 3)
    assert runs == [(b"b", 1), (b"aaccc", 3), (b"", 0)] and GT.layout(runs) == ([0, 16, 32], 21)


def test_argument_errors_without_gpu():
    """validation that returns before any HIP call, in the style of tests/test_abi.py: P / Q stand for an aligned / a misaligned
    pointer, nothing is dereferenced"""
    import ctypes as C
    from ribodetector_amd import _native as N
    L = N.lib()
    P, Q, big = 0x10000, 0x10001, 1 << 40

    def refused(name, args, code, word):
        rc = getattr(L, name)(*args)
        msg = L.rd_last_error()
        assert rc == code and msg.startswith(name.encode() + b":") and word in msg, (name, args, rc, msg)

    def grouped(text=P, tb=1000, n=10, K=4, out=P, tab=P, info=P, ws=P, ws_bytes=big):
        return (text, tb, P, P, n, K, out, 1 << 20, tab, info, ws, ws_bytes, None)
    for name in ("rd_group_pack", "rd_gz_compress_grouped"):
        refused(name, grouped(n=-1), -1, b"bad n")
        refused(name, grouped(tb=-1), -1, b"bad n")
        refused(name, grouped(K=0), -1, b"K = 0")
        refused(name, grouped(K=N.GROUP_KEYS_MAX + 1), -1, b"outside 1..16384")
        refused(name, grouped(info=None), -1, b"null")
        refused(name, grouped(tab=None), -1, b"null")
        refused(name, grouped(text=None), -1, b"null")
        refused(name, grouped(out=None), -1, b"null")
        refused(name, grouped(ws=None), -1, b"null")
        refused(name, grouped(ws=Q), -1, b"aligned")
        refused(name, grouped(out=Q), -1, b"aligned")
        refused(name, grouped(ws_bytes=0), -4, b"workspace too small")
    refused("rd_gz_compress_grouped", grouped(out=P + 16), -1, b"aligned")               # (the deflate's output: 256-byte aligned)
    refused("rd_group_pack", grouped(out=P + 16, ws_bytes=0), -4, b"workspace too small")    # (plain text: 16-byte aligned will do)
    slots = (C.c_int32 * 3)(0, 1, 2)

    def keys(first=0, stride=1, mate=-1, n=10, slot=slots, G=3, info=P):
        return (P, first, stride, mate, P, n, slot, G, P, info, None)
    refused("rd_group_keys", keys(n=-1), -1, b"bad n or G")
    refused("rd_group_keys", keys(G=N.SPLIT_GROUPS_MAX + 1), -1, b"bad n or G")
    refused("rd_group_keys", keys(first=-1), -1, b"first / stride")
    refused("rd_group_keys", keys(stride=0), -1, b"first / stride")
    refused("rd_group_keys", keys(mate=2), -1, b"mate")
    refused("rd_group_keys", keys(slot=None), -1, b"null")
    refused("rd_group_keys", keys(info=None), -1, b"null")
    refused("rd_group_keys", keys(slot=(C.c_int32 * 3)(0, 3, 1)), -1, b"class_slot[1] = 3")
    # the sizes: 0 for what the entry points refuse; the padded stream of the gzip call holds a member per key more than the text's
    assert L.rd_group_workspace_bytes(-1, 10, 4, 0) == 0 and L.rd_group_workspace_bytes(10, -1, 4, 1) == 0
    assert L.rd_group_workspace_bytes(10, 10, 0, 0) == 0 and L.rd_group_workspace_bytes(10, 10, N.GROUP_KEYS_MAX + 1, 1) == 0
    assert 0 < L.rd_group_workspace_bytes(1000, 100000, 50, 0) < L.rd_group_workspace_bytes(1000, 100000, 50, 1)
    # per key more: a member of the padded stream and its slot, and the key's words in the tables (1,024 parts of 12 bytes, and a few)
    a, b = L.rd_group_workspace_bytes(1000000, 250000000, 50, 1), L.rd_group_workspace_bytes(1000000, 250000000, 770, 1)
    assert (770 - 50) * (65280 + 65536) <= b - a <= (770 - 50) * (65280 + 65536 + 1024 * 12 + 64) + 65536
    assert L.rd_gz_grouped_out_bound(-1, 4) == 0 and L.rd_gz_grouped_out_bound(10, 0) == 0
    for tb, K in ((0, 1), (1, 1), (65280, 3), (250000000, 770)):
        assert L.rd_gz_grouped_out_bound(tb, K) == tb + (tb // 65280 + K) * 31 >= L.rd_gz_out_bound(tb)


HDR = b"@HD\tVN:1.6\n@RG\tID:a\n@RG\tID:b/c\n"


def _refused(monkeypatch, tmp_path, argv, msg, env=None, header=HDR):
    """main(argv) ends with the RuntimeError before a Predictor is made (tests/test_bam_host.py's form)"""
    from ribodetector_amd import detect
    bam.write_bam(str(tmp_path / "in.bam"), [], text=header)
    bam.write_bam(str(tmp_path / "in2.bam"), [], text=header)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(detect.Predictor, "__init__", lambda self, *a, **k: pytest.fail("a Predictor was made"))
    argv = ["-l", "100", "--split_groups"] + [a if a.startswith("-") else str(tmp_path / a) for a in argv]
    with pytest.raises(RuntimeError, match=msg) as e:
        detect.main(argv)
    assert "before anything touches a device" in str(e.value)


def test_refusals_before_anything_touches_a_device(monkeypatch, tmp_path):
    import re
    ok = ["-i", "in.bam", "-o", "non.fq.gz"]
    open(str(tmp_path / "in.fq"), "w").write("@r\nACGT\n+\nFFFF\n")
    _refused(monkeypatch, tmp_path, ["-i", "in.fq", "-o", "non.fq"], "every -i file must end with .bam or .ubam")
    _refused(monkeypatch, tmp_path, ok, "duplicate @RG ID 'a'", header=b"@RG\tID:a\n@RG\tID:a\n")
    _refused(monkeypatch, tmp_path, ok, "@RG line without ID", header=b"@RG\tSM:x\n")
    many = b"".join(b"@RG\tID:g%d\n" % k for k in range(1025))
    _refused(monkeypatch, tmp_path, ok, "declares 1025 read groups, more than 1024", header=many)
    _refused(monkeypatch, tmp_path, ["-i", "in.bam", "-o", "n" * 246 + ".fq.gz"], "longer than 255 bytes")
    _refused(monkeypatch, tmp_path, ok + ["--read_report", "non.rg-a.fq.gz"], "two files of the run have the same name")
    _refused(monkeypatch, tmp_path, ok + ["--summary", "non.unassigned.fq.gz"], "two files of the run have the same name")
    _refused(monkeypatch, tmp_path, ok + ["--windows", "--regions", "non.rg-b%2Fc.fq.gz"], "two files of the run have the same name")
    _refused(monkeypatch, tmp_path, ["-i", "in.bam", "-o", "x.fq", "-r", "x.fq"], "two files of the run have the same name")
    _refused(monkeypatch, tmp_path, ok, "deflated on the device only: it cannot run with RD_DEVICE_GZIP=host", env={"RD_DEVICE_GZIP": "host"})
    monkeypatch.delenv("RD_DEVICE_GZIP")
    _refused(monkeypatch, tmp_path, ["-i", "in.bam", "-o", "non.fq"], re.escape("--split_groups under several ranks is not implemented: run on one rank"),
             env={"WORLD_SIZE": "2"})


def test_the_open_file_limit_is_checked_in_a_child_process(tmp_path):
    """files + 64 > soft RLIMIT_NOFILE: refused with both numbers and `ulimit -n` (the limit is lowered in a child process only)"""
    import subprocess
    bam.write_bam(str(tmp_path / "in.bam"), [], text=b"".join(b"@RG\tID:g%d\n" % k for k in range(40)))
    code = ("import resource, sys\n"
            "resource.setrlimit(resource.RLIMIT_NOFILE, (100, resource.getrlimit(resource.RLIMIT_NOFILE)[1]))\n"
            "from ribodetector_amd import detect\n"
            "try:\n"
            "    detect.check_split_groups(True, [sys.argv[1]], [sys.argv[2]], None, 'rrna')\n"
            "except RuntimeError as e:\n"
            "    print(e)\n")
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.bam"), str(tmp_path / "non.fq")], capture_output=True, text=True, cwd=root,
                         timeout=120).stdout
    assert "writes 41 files and needs 105 open files, the limit is 100" in out and "ulimit -n" in out


def test_the_check_passes_and_returns_the_ids_in_row_order(tmp_path):
    from ribodetector_amd import detect
    bam.write_bam(str(tmp_path / "in.bam"), [], text=HDR.replace(b"ID:a", b"ID:z"))
    assert detect.check_split_groups(False, ["x.fq"], ["o.fq"], None, "rrna") is None
    assert detect.check_split_groups(True, [str(tmp_path / "in.bam")], [str(tmp_path / "o.fq")], None, "rrna") == [b"b/c", b"z"]
    fams = detect.split_families(["o1.fq", "o2.fq"], ["r1.fq", "r2.fq"], True, "both")
    assert fams == [(1, ["r1.fq", "r2.fq"]), (0, ["o1.fq", "o2.fq"]), (-1, ["o1.fq.unclassified.gz", "o2.fq.unclassified.gz"])]


def test_600_gzip_writers_of_device_made_members(tmp_path):
    """a run with a file per read group holds hundreds of .gz writers that only ever receive complete members: 600 open at once, 50 of
    them fed with BGZF members - every file is valid gzip afterwards, the fed ones hold their text"""
    import gzip
    from ribodetector_amd.data_loader import fastx_parser as fx
    handles = [fx.open_for_write(str(tmp_path / ("w%03d.fq.gz" % k))) for k in range(600)]
    text = {k: b"@r%d\nACGT\n+\nFFFF\n" % k * (k + 1) for k in range(0, 600, 12)}
    assert len(text) == 50
    for k, t in text.items():
        m = np.frombuffer(bam.bgzf_member(t) + bam.bgzf_member(t[:9]), dtype=np.uint8)
        handles[k].write_members(m.ctypes.data, m.size)
    for h in handles:
        h.close()
    for k in range(600):
        assert gzip.decompress(open(str(tmp_path / ("w%03d.fq.gz" % k)), "rb").read()) == (text[k] + text[k][:9] if k in text else b"")
