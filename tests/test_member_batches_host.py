"""data_loader/member_batches.py on the CPU: the producer loop both BGZF feeders share, and the zlib tail behind it.

The feeders pass gz.DeviceGunzip.index and inflate a batch's members on the GPU; here `index` is rd_host_gz_index over a numpy member
table and zlib inflates every listed member (a row: offset of the DEFLATE data, offset of its text, in_len | out_len << 32). The judges
are the original bytes and BgzfView.text: whatever the block size, the batch sizes and the share, the batches' text [drop, drop + take)
is the share's text."""
import ctypes as C
import gzip
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import deflate_corpus as D
from ribodetector_amd import _native as N
from ribodetector_amd.data_loader import fastx_parser as fx
from ribodetector_amd.data_loader import member_batches as mb

BLOCKS = (40, 700, 65280)
SIZES = ((1, 1 << 17), (50, 1 << 17), (700, 70000), (1 << 20, 1 << 20))      # (first, full); full exceeds the largest member
SLACK = 1 << 17
EMPTY_STORED = b"\x01\x00\x00\xff\xff"       # an empty member that is NOT BGZF's end-of-file block: listed, inflates to nothing
TRUNCATED = "ended before the end-of-stream marker"


def _records(lo, hi, seed=11):
    rng = np.random.default_rng(seed + lo)
    out = []
    for i in range(lo, hi):
        n = int(rng.integers(60, 101))
        out.append(b"@read%d lane %d\n%s\n+\n%s\n" % (i, i % 8, bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)),
                                                      bytes(rng.choice(list(b"FF:,#"), n).astype(np.uint8))))
    return b"".join(out)


def _blocks(text, block, eof=True):
    """BGZF members of `block` text bytes, an empty member sprinkled in after every 7th, BGZF's EOF block last"""
    out = []
    for k, i in enumerate(range(0, len(text), block)):
        out.append(D.sized_member(D.zlib_raw(text[i:i + block]), text[i:i + block]))
        if k % 7 == 3:
            out.append(D.sized_member(EMPTY_STORED, b""))
    return b"".join(out) + (D.sized_member(D.zlib_raw(b""), b"") if eof else b"")


@pytest.fixture(scope="module")
def text():
    t = _records(0, 3000)
    assert 400_000 < len(t) < 700_000
    return t


@pytest.fixture(scope="module")
def bgzf_files(tmp_path_factory, text):
    d = tmp_path_factory.mktemp("member_batches")
    paths = {}
    for block in BLOCKS:
        paths[block] = str(d / ("b%d.fastq.gz" % block))
        Path(paths[block]).write_bytes(_blocks(text, block))
    return paths


class Run:
    """member_batches over one file with two slots, consumed in place: every member of a batch by zlib, every Tail by zlib_member_texts"""

    def __init__(self, path, first, full, span=None, slack=SLACK, stop_at=None):
        self.path, self.first, self.full, self.span, self.slack = path, first, full, span, slack
        self.stop_at = stop_at                       # acquire() answers None from that call on
        self.bufs = [np.zeros(full + slack, dtype=np.uint8) for _ in range(2)]
        self.state = ["free", "free"]                # free -> out (acquired) -> free (released) | consumer (yielded) -> free
        self.tables = [None, None]
        self.acquired = self.batches = 0
        self.pieces = []

    def acquire(self):
        self.acquired += 1
        if self.stop_at is not None and self.acquired >= self.stop_at:
            return None
        assert "out" not in self.state, "a slot was neither released nor yielded before the next was asked for"
        slot = self.state.index("free")
        self.state[slot] = "out"
        return slot

    def release(self, slot):
        assert self.state[slot] == "out"
        self.state[slot] = "free"

    def index(self, buf, have, slot):
        ent = np.zeros((max(1024, have // 64 + 16), 3), dtype=np.int64)
        n, consumed, ob = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = N.host_lib().rd_host_gz_index(buf.ctypes.data, have, 0, 0, ent.ctypes.data, len(ent), C.byref(n), C.byref(consumed), C.byref(ob))
        if rc < 0:
            raise ValueError(N.host_lib().rd_host_last_error().decode())
        self.tables[slot] = ent[:n.value]
        return n.value, consumed.value, ob.value, rc == 1

    def run(self):
        """the text delivered; self.pieces keeps it when an error ends the run"""
        try:
            with open(self.path, "rb", buffering=0) as fh:
                for ev in mb.member_batches(fh, self.index, self.acquire, self.release, self.bufs, self.first, self.full, span=self.span, slack=self.slack):
                    if isinstance(ev, mb.Tail):
                        for out in mb.zlib_member_texts(fh, ev.data):
                            assert isinstance(out, bytes) and 0 < len(out) <= 16 << 20
                            self.pieces.append(out)
                        continue                     # (nothing may follow a Tail: the loop ends by itself)
                    assert self.state[ev.slot] == "out"
                    self.state[ev.slot] = "consumer"
                    ent, buf, at, parts = self.tables[ev.slot], self.bufs[ev.slot], 0, []
                    assert ev.n == len(ent) > 0
                    for in_off, out_off, lens in ent.tolist():
                        in_len, out_len = lens & 0xffffffff, lens >> 32
                        assert out_off == at and in_off + in_len + 8 <= ev.nbytes
                        parts.append(zlib.decompress(buf[in_off:in_off + in_len].tobytes(), -15))
                        assert len(parts[-1]) == out_len
                        at += out_len
                    assert at == ev.out_bytes and 0 <= ev.drop and 0 <= ev.take and ev.drop + ev.take <= ev.out_bytes
                    self.pieces.append(b"".join(parts)[ev.drop:ev.drop + ev.take])
                    self.batches += 1
                    self.state[ev.slot] = "free"
        finally:
            assert self.state == ["free", "free"], self.state        # every slot handed out was released or yielded, once
        return b"".join(self.pieces)


def test_the_module_needs_neither_torch_nor_the_device_bindings():
    code = "import sys; import ribodetector_amd.data_loader.member_batches; assert 'torch' not in sys.modules and 'ribodetector_amd.gz' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(Path(__file__).resolve().parents[1]))


@pytest.mark.parametrize("first,full", SIZES)
@pytest.mark.parametrize("block", BLOCKS)
def test_whole_file_is_the_text(bgzf_files, text, block, first, full):
    r = Run(bgzf_files[block], first, full)
    assert r.run() == text
    assert r.batches >= (2 if first < 1 << 20 else 1)


@pytest.fixture(scope="module")
def shares(bgzf_files, text):
    """{block: (view, {world: [(a, b) per rank]})}: plan_ranges' shares of the text, each checked against BgzfView.text once"""
    out = {}
    for block, path in bgzf_files.items():
        view = fx.BgzfView(path)
        assert view.size == len(text)
        plans = {world: [tuple(fx.plan_ranges([path], rank, world, views=[view])[0]) for rank in range(world)] for world in (1, 2, 3, 5)}
        for ab in plans.values():
            assert ab[0][0] == 0 and ab[-1][1] == len(text) and all(x[1] == y[0] for x, y in zip(ab, ab[1:]))
            assert all(view.text(a, b) == text[a:b] for a, b in ab)
        out[block] = (view, plans)
    return out


@pytest.mark.parametrize("first,full", SIZES)
@pytest.mark.parametrize("block", BLOCKS)
def test_rank_shares_are_their_text_and_add_up(bgzf_files, shares, text, block, first, full):
    view, plans = shares[block]
    for world, ab in plans.items():
        got = [Run(bgzf_files[block], first, full, span=(*view.file_span(a, b), b - a)).run() for a, b in ab]
        assert [len(g) for g in got] == [b - a for a, b in ab]
        assert all(g == text[a:b] for g, (a, b) in zip(got, ab))
        assert b"".join(got) == text


@pytest.fixture(scope="module")
def mixed(text):
    cut1, cut2 = text.index(b"@read1800 "), text.index(b"@read2400 ")
    a, b, c = text[:cut1], text[cut1:cut2], text[cut2:]
    return a, b, c, _blocks(a, 700, eof=False) + gzip.compress(b) + gzip.compress(c)


@pytest.mark.parametrize("first,full", SIZES)
def test_plain_members_and_zero_padding_behind_the_blocks(tmp_path, mixed, first, full):
    a, b, c, blob = mixed
    p = tmp_path / "mixed.fastq.gz"
    p.write_bytes(blob + b"\0" * 4096)
    assert Run(str(p), first, full).run() == a + b + c


def test_truncated_plain_member_behind_the_blocks(tmp_path, mixed):
    a, b, c, blob = mixed
    p = tmp_path / "cut.fastq.gz"
    p.write_bytes(blob + gzip.compress(b"@x\nAC\n+\nFF\n")[:-6])
    r = Run(str(p), 50, 1 << 17)
    with pytest.raises(ValueError, match=TRUNCATED):
        r.run()
    assert b"".join(r.pieces).startswith(a + b + c)      # what lies before the damage was delivered, in order
    p.write_bytes(blob + b"\0" * 4096 + gzip.compress(b"@x\nAC\n+\nFF\n")[:-6])
    with pytest.raises(ValueError, match="incorrect header check"):      # padding is skipped behind the LAST member only
        Run(str(p), 50, 1 << 17).run()


@pytest.mark.parametrize("first,full", SIZES)
def test_truncated_bgzf_file(tmp_path, bgzf_files, text, first, full):
    p = tmp_path / "short.fastq.gz"
    p.write_bytes(Path(bgzf_files[700]).read_bytes()[:-11])
    r = Run(str(p), first, full)
    with pytest.raises(ValueError, match=TRUNCATED):
        r.run()
    assert b"".join(r.pieces) == text


def test_member_larger_than_the_buffer(tmp_path):
    data = bytes(np.random.default_rng(5).integers(0, 256, 60000, dtype=np.uint8))
    p = tmp_path / "big.fastq.gz"
    p.write_bytes(D.sized_member(D.zlib_raw(data), data) + D.sized_member(D.zlib_raw(b""), b""))
    with pytest.raises(ValueError, match="gzip member larger than 1024 bytes"):
        Run(str(p), 1024, 1024, slack=4096).run()


@pytest.mark.parametrize("stop_at", [1, 2, 4])
def test_no_slot_means_stopped(bgzf_files, text, stop_at):
    r = Run(bgzf_files[700], 50, 1 << 17, slack=1024, stop_at=stop_at)       # (batches of 1, 2, 4 KiB: the file is far from over)
    got = r.run()                                        # no exception; what was delivered is a prefix
    assert text.startswith(got) and len(got) < len(text) and r.acquired == stop_at
