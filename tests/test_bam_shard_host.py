"""--bam_shard without a GPU: the rule of bam.find_record_start against the serial walk, data_loader/bam_shard.BamView(device=None)
and the ranges fastx_parser.plan_ranges makes of it, and the argument rules that hold before anything touches a device."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_shard_files as F  # noqa: E402
from ribodetector_amd import _native as N  # noqa: E402
from ribodetector_amd import bam  # noqa: E402
from ribodetector_amd.data_loader import bam_shard  # noqa: E402
from ribodetector_amd.data_loader import fastx_parser as fx  # noqa: E402


# ---- 1. the rule against the serial walk ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    data = bam.payload(F.mixed_reads(11), refs=[(b"chr1", 1 << 20)], text=b"@HD\tVN:1.6\n")
    starts, _ = F.starts_of(data)
    return data, starts


def test_confirm_is_8_everywhere():
    assert bam.CONFIRM == N.BAM_CONFIRM == 8
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ribodetector_amd.h")).read()
    assert "#define RD_BAM_CONFIRM 8" in hdr


def test_an_accepted_start_is_a_record_of_the_walk(mixed):
    data, starts = mixed
    assert len(data) > 300_000 and max(b - a for a, b in zip(starts, starts[1:])) > 100_000      # (the 70 kb records are there)
    ok = set(starts) | {len(data)}
    nxt = np.array(starts + [len(data)])
    rng = np.random.default_rng(12)
    offsets = list(range(4096)) + sorted(int(x) for x in rng.integers(4096, len(data), size=2000))
    for lo in offsets:
        got = F.accepted(data, lo)
        assert got in ok, (lo, got)
        if lo >= starts[0]:          # every record here carries the signature and is < 64 MiB: the FIRST start at or behind lo
            assert got == int(nxt[np.searchsorted(nxt, lo)]), (lo, got)


def test_eight_records_in_a_payload_are_returned_and_seven_are_not():
    data, h0, payload, behind = F.with_host(8)
    assert bam.find_record_start(data, h0 + 1, len(data), True) == (payload, -1)          # the documented false hit
    assert bam.find_record_start(data, payload + 1, len(data), True) == (behind, -1)      # (seven in a row, then noise)
    assert payload not in F.starts_of(data, 0)[0]
    data, h0, payload, behind = F.with_host(7)
    assert bam.find_record_start(data, h0 + 1, len(data), True) == (behind, -1)
    assert behind in F.starts_of(data, 0)[0]


def test_a_window_that_ends_inside_the_chain_is_undecided(mixed):
    data, starts = mixed
    k = 40
    a, b = starts[k], starts[k + 8]                     # eight records: [a, b)
    for end in (b - 1, starts[k + 7] + 36, starts[k + 3] + 2, a + 36, a + 35, a + 1):
        found, und = bam.find_record_start(data[:end], a, end, False)
        assert found == -1 and und == a, (end, found, und)
        assert bam.chain_verdict(data[:end], a, end, False) == bam.UNDECIDED
    assert bam.find_record_start(data[:b], a, b, False)[0] == a          # the eighth record ends with the window: confirmed
    found, und = bam.find_record_start(data[:b], a, b, False)
    assert und > found                                                  # (the last offsets of a window that goes on are always undecided)
    # inside a record, not at_eof: its bytes are rejected, nothing behind them is confirmed yet
    found, und = bam.find_record_start(data[:starts[k + 2]], a + 1, starts[k + 2], False)
    assert found == starts[k + 1] or (found == -1 and und >= 0)


def test_at_eof_confirms_a_short_chain_that_ends_on_the_last_byte(mixed):
    data, starts = mixed
    n = len(data)
    for back in (1, 2, 7):
        a = starts[-back]
        assert bam.find_record_start(data, a, n, True) == (a, -1)
        assert bam.find_record_start(data, a, n, False) == (-1, a)
        assert bam.find_record_start(data[:n - 1], a, n - 1, True) == (-1, -1)          # the file ends inside the last record: rejected
    assert bam.find_record_start(data, starts[-1] + 1, n, True) == (-1, -1)
    assert bam.find_record_start(data, n, n, True) == (-1, -1)


def test_the_signature_tests_what_the_device_tests():
    rec = bytearray(F.DECOY) + bytes(40)
    end = len(rec)
    assert bam.plausible(bytes(rec), 0, end)
    import struct
    for at, v in ((4, -2), (8, -2), (24, -2), (28, -2), (0, 32), (0, (1 << 26) + 1)):
        bad = bytearray(rec)
        struct.pack_into("<i", bad, at, v)
        assert not bam.plausible(bytes(bad), 0, end), (at, v)
    ok = bytearray(rec)
    struct.pack_into("<i", ok, 0, 1 << 26)
    assert bam.plausible(bytes(ok), 0, end)              # (the signature: the record need not lie in the window)
    bad = bytearray(rec)
    bad[12] = 0
    assert not bam.plausible(bytes(bad), 0, end)
    bad = bytearray(rec)
    bad[36 + 5] = 1                                      # the name's NUL
    assert not bam.plausible(bytes(bad), 0, end) and bam.plausible(bytes(bad), 0, 36 + 5)
    bad = bytearray(rec)
    bad[36 + 2] = 32
    assert not bam.plausible(bytes(bad), 0, end) and bam.plausible(bytes(bad), 0, 36 + 2)
    assert not bam.plausible(bytes(rec), 0, 35)


# ---- 2. BamView on the host ---------------------------------------------------------------------------------------------------------------
def _plan(paths, world, views_of):
    res, slots, bar, errs = [None] * world, [None] * world, threading.Barrier(world), []

    def work(r):
        def ag(obj):
            slots[r] = obj
            bar.wait()
            out = list(slots)
            bar.wait()
            return out
        try:
            res[r] = [tuple(x) for x in fx.plan_ranges(paths, r, world, ag, views=views_of())]
        except BaseException as e:      # noqa: BLE001
            errs.append(e)
            bar.abort()
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    if errs:
        raise [e for e in errs if not isinstance(e, threading.BrokenBarrierError)][0]
    return res


@pytest.fixture(scope="module")
def mates(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_shard")
    p1, p2 = str(d / "m_1.bam"), str(d / "m_2.bam")
    d1 = bam.write_bam(p1, F.small_reads(21, 1500, 100, 150, skipped_every=7, prefix=b"a"), member_bytes=4096, text=b"@HD\tVN:1.6\n@CO\tone\n")
    d2 = bam.write_bam(p2, F.small_reads(22, 1500, 30, 60, prefix=b"b"), member_bytes=4096)
    return (p1, d1), (p2, d2)


def test_the_four_answers_agree_with_the_walk(mates):
    (p1, d1), _ = mates
    v = bam_shard.BamView(p1, device=None)
    starts, delivered = F.starts_of(d1)
    hl = bam.header_len(d1)
    assert v.size == len(d1) and v.header_len == hl == starts[0]
    assert v.text(0, v.size) == d1
    nxt = np.array(starts + [len(d1)])
    rng = np.random.default_rng(23)
    for pos in [0, 1, hl - 1, hl, hl + 1, len(d1) - 1, len(d1), len(d1) + 5, starts[-1], starts[-1] + 1] + [int(x) for x in rng.integers(0, len(d1), 60)]:
        want = hl if pos <= hl else len(d1) if pos >= len(d1) else int(nxt[np.searchsorted(nxt, pos)])
        assert v.find_record_start(pos) == want, pos
    dl = np.array(delivered + [False])
    for _ in range(12):
        i, j = sorted(int(x) for x in rng.integers(0, len(starts) + 1, 2))
        assert v.count_records(nxt[i], nxt[j]) == int(dl[i:j].sum()), (i, j)
    assert v.count_records(0, len(d1)) == int(dl.sum()) == 1500 and v.count_records(len(d1), len(d1)) == 0
    dstarts = [s for s, k in zip(starts, delivered) if k]
    ends = {s: int(nxt[starts.index(s) + 1]) for s in dstarts}
    for i, k in ((0, 0), (0, 1), (5, 0), (5, 3), (100, 250), (1400, 100), (1400, 101), (1400, 5000)):
        a = dstarts[i]
        want = a if k == 0 else ends[dstarts[i + k - 1]] if i + k - 1 < len(dstarts) else len(d1)
        assert v.skip_records(a, k) == want, (i, k)
    assert v.skip_records(0, 0) == 0 and v.skip_records(0, 2) == ends[dstarts[1]]
    r = v.make_range(starts[3], starts[9])
    assert isinstance(r, fx.BgzfRange) and r.view is v and tuple(r) == (starts[3], starts[9])


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_plan_ranges_one_file_and_two_mate_files(mates, world):
    (p1, d1), (p2, d2) = mates
    starts1, del1 = F.starts_of(d1)
    for paths, datas in (([p1], [d1]), ([p1, p2], [d1, d2])):
        res = _plan(paths, world, lambda: [bam_shard.BamView(p, device=None) for p in paths])
        held = []
        for f, data in enumerate(datas):
            starts, delivered = F.starts_of(data)
            ok = set(starts) | {len(data), 0}
            at = 0
            idx = []
            for r in range(world):
                a, b = res[r][f]
                assert a == at or (r > 0 and a == b == at) or (at == 0 and a == 0), (world, r, a, at)
                assert a in ok and b in ok and a <= b
                at = b
                lo = sum(1 for s, k in zip(starts, delivered) if k and s < max(a, starts[0]))
                hi = sum(1 for s, k in zip(starts, delivered) if k and s < b)
                idx.append((lo, hi))
            assert res[0][f][0] == 0 and at == len(data)            # the ranges concatenate to the whole stream
            held.append(idx)
        assert all(h == held[0] for h in held), (world, held)        # the same delivered-record indices in both files
        assert held[0][0][0] == 0 and held[0][-1][1] == 1500


def test_more_ranks_than_records_gives_empty_shares(tmp_path):
    p = str(tmp_path / "two.bam")
    data = bam.write_bam(p, F.small_reads(31, 2), member_bytes=4096)
    res = _plan([p], 5, lambda: [bam_shard.BamView(p, device=None)])
    spans = [r[0] for r in res]
    assert spans[0][0] == 0 and spans[-1][1] == len(data) and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    v = bam_shard.BamView(p, device=None)
    counts = [v.count_records(a, b) for a, b in spans]
    assert sum(counts) == 2 and counts.count(0) >= 3
    q = str(tmp_path / "two_2.bam")
    bam.write_bam(q, F.small_reads(32, 2, 20, 30), member_bytes=4096)
    res = _plan([p, q], 5, lambda: [bam_shard.BamView(x, device=None) for x in (p, q)])
    n1 = [v.count_records(*r[0]) for r in res]
    v2 = bam_shard.BamView(q, device=None)
    assert n1 == [v2.count_records(*r[1]) for r in res] and sum(n1) == 2


def test_count_records_across_the_decoy_raises_the_boundary_error(tmp_path):
    host, at = F.decoy_host(8)
    reads = F.small_reads(41, 300) + [host] + F.small_reads(42, 300, prefix=b"u")
    p = str(tmp_path / "decoy.bam")
    data = bam.write_bam(p, reads, member_bytes=4096)
    starts, _ = F.starts_of(data)
    h0 = starts[300]
    v = bam_shard.BamView(p, device=None)
    assert v.find_record_start(h0 + 1) == h0 + at                     # the false hit
    with pytest.raises(ValueError, match="is not a BAM record boundary \\(a byte pattern that looks like 8 records in a row\\): run this file on one rank") as e:
        v.count_records(starts[0], h0 + at)
    assert "offset %d of %s" % (h0 + at, p) in str(e.value)
    with pytest.raises(ValueError, match="not a BAM record boundary"):
        v.count_records(h0 + at, len(data) - 1)
    assert v.count_records(starts[0], starts[301]) == 301             # the same share, cut at the true boundary behind the host


def test_no_record_start_within_the_largest_probe(tmp_path, monkeypatch):
    p = str(tmp_path / "far.bam")
    big = F.read_of(np.random.default_rng(51), 30000, b"big")         # 45 kb
    data = bam.write_bam(p, F.small_reads(52, 3) + [big] * 9, member_bytes=4096)
    starts, _ = F.starts_of(data)
    monkeypatch.setattr(bam_shard.BamView, "PROBE", 1 << 12)
    monkeypatch.setattr(bam_shard.BamView, "PROBE_MAX", 1 << 14)
    v = bam_shard.BamView(p, device=None)
    with pytest.raises(ValueError, match="no BAM record start within \\d+ bytes behind offset %d of " % (starts[3] + 1)):
        v.find_record_start(starts[3] + 1)
    monkeypatch.setattr(bam_shard.BamView, "PROBE_MAX", 1 << 30)
    assert v.find_record_start(starts[3] + 1) == starts[4] and v.stats["probes"] > 2      # the probe grew


# ---- 3. the argument rules ----------------------------------------------------------------------------------------------------------------
BAD_ARGS = [
    (["--bam_shard", "-i", "a.fq", "-o", "o.fq"], {}, "every -i file must end with .bam or .ubam"),
    (["--bam_shard", "-i", "a.fq.gz", "-o", "o.fq"], {"WORLD_SIZE": "2"}, "every -i file must end with .bam or .ubam"),
    (["--bam_shard", "--interleaved", "-i", "a.bam", "-o", "o.fq"], {"WORLD_SIZE": "2"}, "an interleaved BAM is not shared by byte ranges: run on one rank"),
    (["--bam_shard", "-i", "a.bam", "-o", "o.fq"], {"RD_BGZF_SHARD": "0"}, "RD_BGZF_SHARD=0"),
    (["--bam_shard", "-i", "a.bam", "-o", "o.fq"], {"RD_BGZF_SHARD": "0", "WORLD_SIZE": "2"}, "RD_BGZF_SHARD=0"),
    (["-i", "a.bam", "-o", "o.fq"], {"WORLD_SIZE": "2"}, "runs on one rank.*\\(or give --bam_shard"),
    (["--read_groups", "--summary", "s.json", "-i", "a.bam", "-o", "o.fq"], {"WORLD_SIZE": "2"}, "runs on one rank"),
    (["--bam_shard", "-i", "a.bam", "-o", "o.fq"], {"WORLD_SIZE": "2", "RD_DEVICE_PARSE": "0"}, "RD_DEVICE_PARSE=0"),
]
ENV = ("RD_DEVICE_PARSE", "RD_DEVICE_INFLATE", "RD_INGEST", "WORLD_SIZE", "RD_BGZF_SHARD")


@pytest.mark.parametrize("argv,env,msg", BAD_ARGS)
def test_argument_errors_before_anything_touches_a_device(tmp_path, monkeypatch, argv, env, msg):
    from ribodetector_amd import detect
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(detect.Predictor, "__init__", lambda self, *a, **k: pytest.fail("a Predictor was made"))
    monkeypatch.setattr(detect.Predictor, "load_model", lambda self: pytest.fail("the model was loaded"))
    argv = ["-l", "100"] + [a if a.startswith("-") else str(tmp_path / a) for a in argv]
    with pytest.raises(RuntimeError, match=msg) as e:
        detect.main(argv)
    assert "before anything touches a device" in str(e.value)


def test_arguments_accepted(tmp_path, monkeypatch):
    from ribodetector_amd import detect
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    t = lambda name: str(tmp_path / name)      # noqa: E731
    assert detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.fq", "--bam_shard"]).bam_shard is True
    assert detect.build_parser().parse_args(["-l", "100", "-i", "a.bam", "-o", "o.fq"]).bam_shard is False
    assert detect.check_bam([t("a.bam")], [t("o.fq")], None, bam_shard=True) is True                       # one rank: nothing changes
    assert detect.check_bam([t("a.bam")], [t("o.fq")], None, bam_shard=True, interleaved=True) is True
    monkeypatch.setenv("WORLD_SIZE", "3")
    assert detect.check_bam([t("a.bam")], [t("o.fq")], None, bam_shard=True) is True
    assert detect.check_bam([t("a.bam"), t("b.ubam")], [t("o1.bam"), t("o2.bam")], None, bam_output=True, bam_shard=True) is True
    monkeypatch.setenv("RD_BGZF_SHARD", "1")
    assert detect.check_bam([t("a.bam")], [t("o.fq.gz")], [t("r.fq")], bam_shard=True) is True
    bam.write_bam(t("g.bam"), F.small_reads(61, 3, groups=2), text=b"@RG\tID:g00\n@RG\tID:g01\n")
    got = detect.check_read_groups(True, t("s.json"), [t("g.bam")], bam_shard=True)                         # the flag lifts the one-rank rule
    assert [g[0] for g in got] == [b"g00", b"g01"]
    # a rank's part of a BAM output keeps the extension by which the writer makes BGZF blocks
    assert detect.part_path("out/n.bam", 2) == "out/n.part2.bam" and detect.part_path("o.ubam", 0) == "o.part0.ubam"
    assert detect.part_path(detect.unclassified_path("o.bam", True), 1) == "o.bam.unclassified.part1.bam"


def test_the_errors_of_a_share_name_the_cut_or_the_share():
    from ribodetector_amd.data_loader import device_reader as dr
    share = (5000, 90000, 200000)
    e = dr._share_error(ValueError(bam.TRUNCATED), N.BAM_TRUNCATED, share, "x.bam", 1)
    assert str(e).startswith(bam.NOT_A_BOUNDARY % (90000, "x.bam", 8)) and "rank 2" in str(e)
    e = dr._share_error(ValueError(bam.TRUNCATED), N.BAM_TRUNCATED, (5000, 200000, 200000), "x.bam", 1)
    assert str(e) == bam.TRUNCATED                                   # the last share: the file itself ends inside a record
    e = dr._share_error(ValueError(bam.MALFORMED % 7), N.BAM_RECORD, share, "x.bam", 1)
    assert str(e) == "malformed BAM record 7 of the share of rank 1 that starts at inflated offset 5000 of x.bam"
