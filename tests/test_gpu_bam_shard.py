"""--bam_shard on the GPU: rd_bam_find_start against the rule (bam.find_record_start), rd_bam_count against rd_bam_index, BamView on the
device against BamView(device=None), and the CLI under torch.distributed.run against a one-rank run of the same arguments."""
import gzip
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_shard_files as F  # noqa: E402
import bam_windows as W  # noqa: E402
import test_gpu_bam as G  # noqa: E402
import test_gpu_bam_index as I  # noqa: E402,E741
import test_gpu_bam_output as O  # noqa: E402
import test_gpu_cli as CLI  # noqa: E402
from ribodetector_amd import _native as N  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = W.S
CAND = 4096                       # BAM_FIND_CAND: candidates per workgroup of rd_bam_find_kernel (csrc/rd_bam_shard.hpp)


# ---- 5. rd_bam_find_start = the rule ----------------------------------------------------------------------------------------------------
class Finder:
    """one device copy of a window, any number of (lo, hi, end, at_eof) questions: the bytes behind `end` are a canary that carries the
    signature of nothing (0xA5), and the buffer ends at the 16-byte boundary behind the window"""

    def __init__(self, window):
        import torch
        self.window = bytes(window)
        self.dev = torch.device(DEV)
        n = len(self.window)
        self.text = torch.full((max(16, (n + 15) // 16 * 16),), 0xA5, dtype=torch.uint8, device=self.dev)
        if n:
            self.text[:n] = torch.from_numpy(np.frombuffer(self.window, np.uint8).copy()).to(self.dev)
        self.info = torch.empty(4, dtype=torch.int64, device=self.dev)

    def ask(self, lo, hi, end=None, at_eof=False):
        import torch
        end = len(self.window) if end is None else end
        self.info.fill_(77)
        N.check(N.lib().rd_bam_find_start(N.ptr(self.text), lo, hi, end, 1 if at_eof else 0, N.ptr(self.info), N.stream_ptr(self.dev)), "rd_bam_find_start")
        torch.cuda.synchronize()
        return [int(x) for x in self.info.cpu()]

    def same(self, lo, hi, end=None, at_eof=False, tag=""):
        end = len(self.window) if end is None else end
        got = self.ask(lo, hi, end, at_eof)
        want = bam.find_record_start(self.window[:end], lo, hi, at_eof)
        assert (got[0], got[1]) == want and got[2] == got[3] == 0, (tag, lo, hi, end, at_eof, got, want)
        return want


def _three():
    rng = np.random.default_rng(1)
    return b"".join(bam.encode_record(F.read_of(rng, n, b"three%d" % n)) for n in (20, 0, 33))


def test_three_records_every_lo_and_every_way_to_ask():
    w = _three()
    f = Finder(w)
    n = len(w)
    for at_eof in (False, True):
        for lo in range(n + 1):
            f.same(lo, n, at_eof=at_eof)
    assert f.same(0, n, at_eof=True) == (0, -1) and f.same(0, n)[0] == -1
    rng = np.random.default_rng(2)
    for _ in range(60):                                  # hi < end, end < the window
        end = int(rng.integers(0, n + 1))
        lo, hi = sorted(int(x) for x in rng.integers(0, end + 1, 2))
        f.same(lo, hi, end, bool(rng.integers(0, 2)))
    for lo, hi, end in ((0, 0, 0), (n, n, n), (5, 5, n), (0, 0, n)):      # an empty window, lo == end, no candidate
        assert f.same(lo, hi, end, True) == (-1, -1) and f.same(lo, hi, end, False) == (-1, -1)
    for lo, hi, end in ((-1, 5, n), (6, 5, n), (0, n + 1, n), (0, 5, -1)):  # bad arguments: nothing searched
        got = f.ask(lo, hi, end)
        assert got[3] != 0 and got[0] == got[1] == -1, got


@pytest.fixture(scope="module")
def chain():
    """records for 5 workgroups of candidates, one starting exactly at 2 CAND + 1000"""
    c = W.Chain(3).to(2 * CAND + 1000)
    for _ in range(12):
        c.read()
    data = c.to(5 * CAND + 777).window().data
    return Finder(data), 2 * CAND + 1000


@pytest.mark.parametrize("j", [0, 1, 63, 64, 65, 127, 128, CAND - 1, CAND, CAND + 1])
def test_a_true_start_at_every_place_of_a_workgroup(chain, j):
    f, t = chain
    n = len(f.window)
    found = f.same(t - j, n, at_eof=True, tag="start at candidate %d" % j)[0]
    assert found <= t                                    # (a filler in front of t may start in [t - j, t))
    assert f.same(t - j, t + 1, at_eof=True)[0] == found
    if j:
        f.same(t - j, t, at_eof=True)                    # hi excludes the start
    f.same(t - j, n)


@pytest.mark.parametrize("d", W.REACH_D)
@pytest.mark.parametrize("how", ["mid", "cut"])
def test_a_255_byte_name_across_the_end_of_the_stage(d, how):
    """the record with l_read_name = 255 starts d bytes in front of the end of a workgroup's candidates: its fixed fields or its name
    lie in the BAM_REACH bytes staged behind them - or the window ends inside its name"""
    w = W.reach(CAND, d, how)
    f = Finder(w.data)
    n = len(w.data)
    for at_eof in (False, True):
        for lo in (0, CAND - d - 1, CAND - d, CAND - d + 1):
            f.same(lo, n, at_eof=at_eof, tag=how)
        f.same(0, CAND - d + 1, at_eof=at_eof)
    if how == "mid":
        assert f.same(CAND - d, n, at_eof=True)[0] == CAND - d


def test_block_size_limits_and_far_fields():
    rng = np.random.default_rng(4)
    rec = bytearray(bam.encode_record(F.read_of(rng, 50, b"limit")))
    tail = b"".join(bam.encode_record(F.read_of(rng, 40, b"after%d" % i)) for i in range(9))
    for block, want_und in ((1 << 26, True), ((1 << 26) + 1, False), (32, False), (33, False)):
        r = bytearray(rec)
        struct.pack_into("<i", r, 0, block)
        f = Finder(bytes(r) + tail)
        n = len(f.window)
        found, und = f.same(0, n)
        assert (und == 0) == want_und, (block, found, und)         # 2^26: the signature holds, the record ends behind the window
        assert f.same(0, n, at_eof=True)[0] != 0
        assert f.same(0, 1, at_eof=True) == (-1, -1)
    for at in (4, 8, 24, 28):                                # refID / pos / next_refID / next_pos = -2
        r = bytearray(rec)
        struct.pack_into("<i", r, at, -2)
        f = Finder(bytes(r) + tail)
        assert f.same(0, 1, at_eof=True) == (-1, -1)
        assert f.same(0, len(f.window), at_eof=True)[0] == len(r)
    w = W.guess_proof("far_fields").data[:3 * CAND]
    assert Finder(w).same(0, len(w), at_eof=True) == (-1, -1)
    assert Finder(w).same(0, len(w))[0] == -1


def test_decoys_undecided_and_at_eof():
    for k in (8, 7):
        data, h0, payload, behind = F.with_host(k)
        f = Finder(data)
        n = len(data)
        assert f.same(h0 + 1, n, at_eof=True)[0] == (payload if k == 8 else behind)
        assert f.same(payload + 1, n, at_eof=True)[0] == behind
        f.same(0, n)
        f.same(h0 + 1, n)
    data = bam.payload(F.mixed_reads(11, n=200, big=0))
    starts, _ = F.starts_of(data)
    k = 40
    a, b = starts[k], starts[k + 8]
    for end in (b - 1, starts[k + 7] + 36, starts[k + 3] + 2, a + 36, a + 35, a + 1):
        f = Finder(data[:end])
        assert f.same(a, end) == (-1, a)
        f.same(a, end, at_eof=True)
        f.same(0, end)
    assert Finder(data[:b]).same(a, b)[0] == a
    f, n = Finder(data), len(data)
    for back in (1, 2, 7):
        a = starts[-back]
        assert f.same(a, n, at_eof=True) == (a, -1) and f.same(a, n) == (-1, a)
        assert f.same(a, n - 1, n - 1, at_eof=True) == (-1, -1)
    assert f.same(starts[-1] + 1, n, at_eof=True) == (-1, -1)


def test_seeded_sweep():
    """200 (window, lo) pairs: 10 windows of at most 256 KiB that mix reads, fillers, decoys, tiny records, 255-byte names, starts no
    signature finds and records that span workgroups, cut at random; 20 questions each"""
    rng = np.random.default_rng(5)
    for wi in range(10):
        c = W.Chain(rng)
        total = int(rng.integers(3 * CAND, (256 << 10) - 8000))
        enc_u = lambda r: bam.encode_record(W.unprintable(r, rng))      # noqa: E731
        while c.at < total - 12000:
            what = int(rng.integers(0, 8))
            k = c.at // CAND + 2
            if what == 0:
                c.to(c.at + int(rng.integers(2000, 9000)))
            elif what == 1:
                c.to(k * CAND + int(rng.integers(-4, 5))).read()
            elif what == 2:
                c.decoy(k * CAND + int(rng.integers(0, 100)), bool(rng.integers(0, 2)))
            elif what == 3:
                c.span(c.at, int(rng.integers(CAND, 3 * CAND)))
            elif what == 4:
                c.to(c.at + int(rng.integers(1000, 6000)), encode=enc_u if rng.integers(0, 2) else W.far_fields)
            elif what == 5:
                for r in W.tiny(int(rng.integers(10, 300)), named=bool(rng.integers(0, 2))):
                    c.add(r)
            elif what == 6:
                c.to(k * CAND - int(rng.choice(W.REACH_D))).add(W.long_name())
            else:
                for _ in range(9):
                    c.read()
        data = c.window().data
        cut = len(data) if rng.integers(0, 3) == 0 else int(rng.integers(len(data) // 2, len(data)))
        f = Finder(data[:cut])
        assert cut <= 256 << 10
        for _ in range(20):
            lo = int(rng.integers(0, cut + 1))
            hi = cut if rng.integers(0, 3) else int(rng.integers(lo, cut + 1))
            end = cut if rng.integers(0, 4) else int(rng.integers(hi, cut + 1))
            f.same(lo, hi, end, bool(rng.integers(0, 2)), tag="window %d" % wi)


# ---- 6. rd_bam_count = rd_bam_index, field for field ---------------------------------------------------------------------------------------
WORDS = ("status", "dirty", "n_records", "n_lines", "consumed", "bad_record", "reserved", "carry")


def _count(window, final, prev=None):
    import torch
    from ribodetector_amd.data_loader.device_reader import PAD
    lib, dev = N.lib(), torch.device(DEV)
    pad = PAD if prev is not None else 64
    end = pad + len(window)
    text = torch.zeros(((end + 64 + 127) // 64) * 64, dtype=torch.uint8, device=dev)
    if len(window):
        text[pad:end] = torch.from_numpy(np.frombuffer(window, np.uint8).copy()).to(dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    need = int(lib.rd_bam_count_workspace_bytes(end))
    assert 0 < need < int(lib.rd_bam_index_workspace_bytes(end))
    ws = torch.full((max(need, 256) + 256,), 0xA5, dtype=torch.uint8, device=dev)
    for _ in range(2):
        N.check(lib.rd_bam_count(N.ptr(text), pad, end, N.ptr(prev[0]) if prev else None, N.ptr(prev[1]) if prev else None, final, N.ptr(summary), N.ptr(ws),
                                 max(need, 256), N.stream_ptr(dev)), "rd_bam_count")
        torch.cuda.synchronize()
    assert bool((ws[max(need, 256):] == 0xA5).all()), "bytes written behind the workspace"
    begin, wend, n_lines, n, consumed, bad, sd, reserved = (int(x) for x in summary.cpu().numpy())
    assert wend == end
    return dict(status=sd & 0xffffffff, dirty=(sd >> 32) & 0xffffffff, n_records=n, n_lines=n_lines, consumed=consumed - begin, bad_record=bad, reserved=reserved,
                carry=pad - begin, chain=(text, summary))


def _both(window, final, prev_c=None, prev_i=None, tag=""):
    c, i = _count(window, final, prev_c), I._frame(window, final, prev=prev_i)
    for k in WORDS:
        assert c[k] == i[k], (tag, k, c[k], i[k])
    return c, i


def test_count_equals_index_on_one_batch_and_past_64_segments():
    for final in (0, 1):
        c, _ = _both(W.Chain(6).to(3 * S - 100).window().data, final, tag="one batch")
        assert c["status"] == 0 and c["n_lines"] > 20
        _both(b"", final, tag="empty")
    w = W.round_edge(64 * S + S // 2 + 7)
    c, _ = _both(w.data, 1, tag="past 64 segments")
    assert c["consumed"] == len(w.data) and w.nseg > 64
    _both(W.decoys((63, 65), (False, True), n=67).data, 1, tag="decoys")


def test_count_equals_index_on_two_chained_batches():
    w, at, size = W.ends_chain()
    data, cut = w.data, at + size // 2
    c1, i1 = _both(data[:cut], 0, tag="first")
    assert c1["consumed"] == at
    c2, i2 = _both(data[cut:], 1, c1["chain"], i1["chain"], tag="second")
    assert c2["carry"] == cut - at and c2["status"] == 0
    whole = W.expect(data, 1)
    assert c1["n_records"] + c2["n_records"] == whole["n_records"] and c1["n_lines"] + c2["n_lines"] == whole["n_lines"]


@pytest.mark.parametrize("what", ["no_nul", "block=31", "cut_in_record", "cut_in_block_size"])
def test_count_equals_index_on_damage(what):
    w = W.damaged(what).data
    for final in (0, 1):
        c, _ = _both(w, final, tag=what)
        want = W.expect(w, final)
        assert c["status"] == want["status"] and (c["status"] != N.BAM_RECORD or c["bad_record"] == want["bad_record"])
    assert c["status"] in (N.BAM_RECORD, N.BAM_TRUNCATED)


# ---- 7. BamView on the device = BamView on the host -----------------------------------------------------------------------------------------
def test_bam_view_on_the_device_equals_the_host(tmp_path, monkeypatch):
    import torch
    from ribodetector_amd.data_loader import bam_shard
    host, at = F.decoy_host(8)
    big = W.filler(3 << 20, name=b"threeMB")
    reads = F.small_reads(71, 1000, skipped_every=9) + [big] + F.small_reads(72, 700, prefix=b"u") + [host] + F.small_reads(73, 300, prefix=b"v")
    p = str(tmp_path / "v.bam")
    data = bam.write_bam(p, reads, member_bytes=4096, text=b"@HD\tVN:1.6\n")
    hl = bam.header_len(data)
    monkeypatch.setattr(bam_shard.BamView, "BATCH", 1 << 14)            # several chained batches; the 3 MB record spans many of them
    vh, vd = bam_shard.BamView(p, device=None), bam_shard.BamView(p, device=torch.device(DEV))
    assert vd.size == vh.size == len(data) and vd.header_len == vh.header_len == hl
    big_at = data.index(b"threeMB") - 36
    h0 = data.index(b"host\0") - 36
    rng = np.random.default_rng(74)
    asks = [0, hl, hl + 1, big_at, big_at + 1, big_at + (1 << 20), big_at + len(big) - 1, big_at + len(big), h0 + 1, h0 + at, h0 + at + 1, len(data) - 1, len(data)]
    answers = []
    for pos in asks + [int(x) for x in rng.integers(0, len(data), 25)]:
        a = vd.find_record_start(pos)
        assert a == vh.find_record_start(pos), pos
        answers.append(a)
    before = vd.stats["probes"]
    assert vd.find_record_start(big_at + 1) == big_at + len(big) and vd.stats["probes"] >= before + 2         # (the probe had to grow)
    assert vd.find_record_start(h0 + 1) == h0 + at                                                            # the false hit, on both
    true = sorted(set(a for a in answers if a != h0 + at))
    for a, b in [(0, len(data)), (hl, big_at), (big_at, big_at + len(big)), (true[1], true[-2]), (true[3], true[3])] + list(zip(true[2:8], true[3:9])):
        assert vd.count_records(a, b) == vh.count_records(a, b), (a, b)
    before = vd.stats["count_batches"]
    assert vd.count_records(0, len(data)) == 2000 + 1 + 1 and vd.stats["count_batches"] >= before + 8
    for v in (vd, vh):
        with pytest.raises(ValueError, match="offset %d of .* is not a BAM record boundary" % (h0 + at)):
            v.count_records(hl, h0 + at)
        with pytest.raises(ValueError, match="is not a BAM record boundary"):
            v.count_records(big_at + 1, h0)
    for a, k in ((0, 0), (hl, 1), (true[2], 40), (big_at, 1), (true[-2], 10 ** 6)):
        assert vd.skip_records(a, k) == vh.skip_records(a, k)
    assert tuple(vd.make_range(true[1], true[2])) == tuple(vh.make_range(true[1], true[2]))


# ---- 8. the CLI under torch.distributed.run ------------------------------------------------------------------------------------------------
def _synth_reads(n, seed, lengths=(60, 150), mate=None, groups=0):
    from ribodetector_amd import synth
    a, o, _ = synth.reads_numpy(n, lengths, seed=seed, rrna_frac=0.35)
    reads = G._bam_reads(a, o, mate=mate, rng=np.random.default_rng(seed))
    if groups:
        for i, r in enumerate(reads):
            r["tags"] = b"RGZg%02d\0" % (i * 7 % groups) if i % 11 else b""
    return reads


def _shares(text):
    return re.findall(r"Rank (\d) parses ([\d, ]+) bytes of ([\d, ]+) \(decompressed; BGZF members\)", text)


def _no_leftovers(d):
    assert not [f for f in os.listdir(d) if ".part" in f or ".joining" in f]


def test_cli_single_end_two_ranks_and_the_flag_on_one_rank(tmp_path):
    """(a) W = 2: plain and .gz outputs, the report and the summary with its read groups equal one rank's; (e) one rank with the flag
    writes what one rank without it writes"""
    groups = 24
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@RG\tID:g%02d\tSM:s%d\n" % (g, g % 3) for g in range(groups))
    inp = str(tmp_path / "in.bam")
    data = bam.write_bam(inp, _synth_reads(4000, 81, groups=groups), member_bytes=4096, text=text)
    runs = {}
    for tag, flag, world in (("plain", [], 1), ("one", ["--bam_shard"], 1), ("two", ["--bam_shard"], 2)):
        d = tmp_path / tag
        d.mkdir()
        files = [str(d / x) for x in ("x.fq", "y.fq.gz", "rep.tsv", "s.json")]
        args = ["-l", "100", "-i", inp, "-o", files[0], "-r", files[1], "--read_report", files[2], "--summary", files[3], "--read_groups"] + flag + G.SMALL
        if world == 1:
            p = G._run(args)
            assert p.num_read == 4000 and p.num_rrna > 500 and p.num_nonrrna > 500
        else:
            r, _ = CLI._torchrun(world, args, timeout=600)
            out = r.stdout + r.stderr
            assert r.returncode == 0, out[-3000:]
            rows = _shares(out)
            assert sorted(int(x[0]) for x in rows) == list(range(world)) and sum(int(x[1]) for x in rows) == len(data) == int(rows[0][2])
            assert "BAM input: 4000 records, 0 secondary/supplementary skipped" in out
        _no_leftovers(d)
        doc = json.load(open(files[3]))
        runs[tag] = [open(files[0], "rb").read(), gzip.decompress(open(files[1], "rb").read()), open(files[2], "rb").read(), doc]
    assert open(str(tmp_path / "plain" / "y.fq.gz"), "rb").read() == open(str(tmp_path / "one" / "y.fq.gz"), "rb").read()      # (e): the bytes of the .gz too
    for tag in ("one", "two"):
        for k in range(3):
            assert runs[tag][k] == runs["plain"][k] and len(runs[tag][k]) > 0, (tag, k)
        assert runs[tag][3] == runs["plain"][3], tag
    rg = runs["two"][3]["read_groups"]
    assert len(rg["groups"]) == groups and sum(g["units"]["total"] for g in rg["groups"]) + rg["none"]["units"]["total"] == 4000


def test_cli_two_mate_files_three_ranks_bam_output(tmp_path):
    """(b) W = 3, mates of different record sizes (and supplementary records in mate 1 only), -e both --bam_output: every output is the
    input's header, the records one rank selects, and one end-of-file member"""
    n = 4000
    r1 = _synth_reads(n, 82, (100, 150), mate=1)
    r2 = _synth_reads(n, 83, (60, 90), mate=2)
    rng = np.random.default_rng(84)
    r1 = O._tagged(r1, rng, skipped=True)
    i1, i2 = str(tmp_path / "m_1.bam"), str(tmp_path / "m_2.bam")
    d1 = bam.write_bam(i1, r1, member_bytes=4096, text=b"@HD\tVN:1.6\n@CO\tmate 1\n", refs=[(b"chr1", 1000)])
    d2 = bam.write_bam(i2, r2, member_bytes=4096, text=b"@CO\tmate 2\n")
    outs = {}
    for tag, world in (("one", 1), ("three", 3)):
        d = tmp_path / tag
        d.mkdir()
        o, r = [str(d / ("o%d.bam" % k)) for k in (1, 2)], [str(d / ("r%d.ubam" % k)) for k in (1, 2)]
        args = ["-l", "100", "-i", i1, i2, "-o", *o, "-r", *r, "-e", "both", "--bam_output", "--bam_shard"] + G.SMALL
        if world == 1:
            assert G._run(args).num_read == n
        else:
            res, _ = CLI._torchrun(world, args, timeout=600)
            out = res.stdout + res.stderr
            assert res.returncode == 0, out[-3000:]
            rows = _shares(out)
            assert len(rows) == world
            assert sum(int(x[1].split(", ")[0]) for x in rows) == len(d1) and sum(int(x[1].split(", ")[1]) for x in rows) == len(d2)
            assert "BAM input: %d records, %d secondary/supplementary skipped" % (len(r1), len(r1) - n) in out
        _no_leftovers(d)
        outs[tag] = o + r + [x + ".unclassified.bam" for x in o]
    total = 0
    for k, (a, b) in enumerate(zip(outs["one"], outs["three"])):
        src, data = (i1, d1) if k % 2 == 0 else (i2, d2)
        got, want = O._inflate(b), O._inflate(a)           # (_inflate: BGZF members, the end-of-file member once, last)
        hdr = bam.header(src)
        assert got[:len(hdr)] == hdr and got == want, b
        index = {rec.name: j for j, rec in enumerate(x for x in bam.records(data) if not x.skipped)}
        keep = [index[rec.name] for rec in bam.records(want)]
        assert got[len(hdr):] == bam.select(data, keep)
        total += len(keep)
    assert total == 2 * n


def test_cli_more_ranks_than_records(tmp_path):
    """(c) W = 3 on a file of 2 records: the ranks without a share take part in every collective and write empty parts"""
    inp = str(tmp_path / "two.bam")
    bam.write_bam(inp, _synth_reads(2, 85), member_bytes=4096)
    files = {}
    for tag, world in (("one", 1), ("three", 3)):
        d = tmp_path / tag
        d.mkdir()
        files[tag] = [str(d / x) for x in ("x.fq", "y.fq.gz", "rep.tsv")]
        args = ["-l", "100", "-i", inp, "-o", files[tag][0], "-r", files[tag][1], "--read_report", files[tag][2], "--bam_shard"] + G.SMALL
        if world == 1:
            assert G._run(args).num_read == 2
        else:
            res, _ = CLI._torchrun(world, args, timeout=600)
            assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
            assert "BAM input: 2 records" in res.stdout + res.stderr
        _no_leftovers(d)
    for a, b in zip(files["one"], files["three"]):
        assert G._read(a) == G._read(b)
    assert len(G._read(files["one"][0])) + len(G._read(files["one"][1])) > 0


def test_cli_a_cut_in_front_of_the_decoy_fails_cleanly(tmp_path):
    """(d) W = 2 on a file whose midpoint lies in a record that holds 8 records in a tag, just in front of them: rank 1's share would
    start at the first of the 8, rank 0's chain cannot land there - the run fails with the boundary message, no output is joined"""
    host, at = F.decoy_host(8, noise=False)              # (the 8th ends with the host: rank 1's chain goes on along the true one)
    host = bytearray(host)
    struct.pack_into("<H", host, 18, 0x800)              # supplementary: in no output, on one rank
    head = _synth_reads(1500, 86)
    hdr = bam.encode_header(text=b"@HD\tVN:1.6\n")
    h0 = len(hdr) + sum(len(bam.encode_record(r)) for r in head)
    tail, have = [], 0
    lo_t = h0 + 2 - len(host) + 20                       # the tail's bytes: the midpoint falls in (h0, h0 + at], 10 bytes clear of either end
    for r in _synth_reads(2500, 87):
        if lo_t - have < 700:
            break
        tail.append(r)
        have += len(bam.encode_record(r))
    tail.append(F.skipped_filler(lo_t - have))
    inp = str(tmp_path / "decoy.bam")
    data = bam.write_bam(inp, head + [bytes(host)] + tail, member_bytes=4096, text=b"@HD\tVN:1.6\n")
    assert h0 < len(data) // 2 <= h0 + at and bam.find_record_start(data, len(data) // 2, len(data), True)[0] == h0 + at
    one, two = str(tmp_path / "one.fq"), str(tmp_path / "two.fq")
    p = G._run(["-l", "100", "-i", inp, "-o", one, "--bam_shard"] + G.SMALL)
    assert p.num_read == len(head) + len(tail) - 1 and os.path.getsize(one) > 0
    res, _ = CLI._torchrun(2, ["-l", "100", "-i", inp, "-o", two, "--bam_shard"] + G.SMALL, timeout=600)
    out = res.stdout + res.stderr
    assert res.returncode != 0
    assert "the share boundary at offset %d of %s is not a BAM record boundary (a byte pattern that looks like 8 records in a row): run this file on one rank" % (
        h0 + at, inp) in out, out[-3000:]
    assert not os.path.exists(two)
    _no_leftovers(tmp_path)


def test_cli_a_plain_gzip_member_is_refused_by_every_rank(tmp_path):
    """a BAM file whose second half is ONE plain gzip member is not shared by BGZF members: every rank raises, from the broadcast index"""
    reads = _synth_reads(400, 88)
    data = bam.payload(reads, text=b"@HD\tVN:1.6\n")
    half = len(data) // 2
    inp = str(tmp_path / "plain_member.bam")
    with open(inp, "wb") as fh:
        for p in range(0, half, 4096):
            fh.write(bam.bgzf_member(data[p:min(p + 4096, half)]))
        fh.write(gzip.compress(data[half:], 6))
        fh.write(bam.EOF_MEMBER)
    one, two = str(tmp_path / "one.fq"), str(tmp_path / "two.fq")
    assert G._run(["-l", "100", "-i", inp, "-o", one, "--bam_shard"] + G.SMALL).num_read == 400
    res, _ = CLI._torchrun(2, ["-l", "100", "-i", inp, "-o", two, "--bam_shard"] + G.SMALL, timeout=600)
    out = res.stdout + res.stderr
    assert res.returncode != 0 and len(re.findall(r"RuntimeError: --bam_shard: .*not BGZF all the way - run on one rank", out)) >= 1, out[-3000:]
    assert "Rank 0 parses" not in out                        # (raised from the index, before any share is planned)
    assert not os.path.exists(two)
    _no_leftovers(tmp_path)
