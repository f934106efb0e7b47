"""rd_bam_raw_tab / rd_bam_raw_gather below the reader (csrc/rd_bam_raw.hpp): rd_bam_index on a window of raw record bytes, the way
tests/test_gpu_bam_index.py drives it, then the raw view of its delivered records. The expectation is the rule's serial walk alone:
offset and size of every record of bam.records that is not skipped (bam.select joins exactly those bytes).

Every gather goes into an arena pre-filled with 0xA5 with guard bytes behind its capacity, and is compared as a WHOLE arena: the bytes
of the piece where they belong and every other byte - in front of *cursor_in, behind *cursor_out, behind the capacity - as it was."""
import gzip
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_windows as W  # noqa: E402
from ribodetector_amd import _native as N  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = W.S
LINES = 5                         # RD_FQ_LINES
GUARD = 64
FILL, CANARY32, CANARY64 = 0xA5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
EVERY = 4


def _walk(data):
    """(offset, size) of the delivered records of the rule's walk from offset 0, up to the damage if there is one"""
    out = []
    try:
        for r in bam.records(data, start=0):
            if not r.skipped:
                out.append((r.offset, r.size))
    except ValueError:
        pass
    return out


class _Batch:
    pass


def _index(window, final, prev=None, cap_records=None):
    """rd_bam_index on `window` (prev: the batch it chains to), rd_bam_index_src, rd_bam_raw_tab - called twice into the same tables"""
    import torch
    from ribodetector_amd.data_loader.device_reader import PAD
    lib, dev = N.lib(), torch.device(DEV)
    st = N.stream_ptr(dev)
    b = _Batch()
    pad = PAD if prev is not None else 64
    end = pad + len(window)
    b.text = torch.zeros(((end + 64 + 127) // 64) * 64, dtype=torch.uint8, device=dev)
    if len(window):
        b.text[pad:end] = torch.from_numpy(np.frombuffer(window, np.uint8).copy()).to(dev)
    size = len(window) + (pad if prev is not None else 0)
    b.cap = cap = size // 37 + 2 if cap_records is None else cap_records
    ncap = ((4 * size // 3 + 64 + 255) // 256) * 256
    b.norm = torch.empty(ncap, dtype=torch.uint8, device=dev)
    b.rec_tab = torch.empty(cap, dtype=torch.int64, device=dev)
    b.hdr_tab = torch.empty(cap, dtype=torch.int32, device=dev)
    b.summary = torch.zeros(8, dtype=torch.int64, device=dev)
    b.ws = torch.empty(max(int(lib.rd_bam_index_workspace_bytes(end)), 256), dtype=torch.uint8, device=dev)
    N.check(lib.rd_bam_index(N.ptr(b.text), pad, end, N.ptr(prev.text) if prev else None, N.ptr(prev.summary) if prev else None, final, N.ptr(b.norm), ncap,
                             N.ptr(b.rec_tab), N.ptr(b.hdr_tab), cap, N.ptr(b.summary), N.ptr(b.ws), b.ws.numel(), st), "rd_bam_index")
    src = lib.rd_bam_index_src(N.ptr(b.ws), end)
    assert src and b.ws.data_ptr() <= src < b.ws.data_ptr() + b.ws.numel() and src % 4 == 0
    assert lib.rd_bam_index_src(None, end) is None and lib.rd_bam_index_src(N.ptr(b.ws), -1) is None
    b.src = N.C.c_void_p(src)
    b.ns = ns = cap // EVERY + 3
    b.raw_tab = torch.full((cap + GUARD,), CANARY64, dtype=torch.int64, device=dev)
    b.samples = torch.full((ns + GUARD,), CANARY32, dtype=torch.int32, device=dev)
    snaps = []
    for _ in range(2):
        N.check(lib.rd_bam_raw_tab(N.ptr(b.text), b.src, N.ptr(b.summary), N.ptr(b.raw_tab), cap, EVERY, N.ptr(b.samples), ns, st), "rd_bam_raw_tab")
        torch.cuda.synchronize()
        snaps.append((b.raw_tab.cpu().numpy().copy(), b.samples.cpu().numpy().copy()))
    assert np.array_equal(snaps[0][0], snaps[1][0]) and np.array_equal(snaps[0][1], snaps[1][1]), "a second call changed the tables"
    b.tab, b.smp = snaps[0]
    assert (b.tab[cap:] == CANARY64).all() and (b.smp[ns:] == CANARY32).all(), "entries written behind the tables"
    h = b.summary.cpu().numpy()
    b.begin, b.end, b.n, b.consumed, b.status = int(h[0]), int(h[1]), int(h[3]), int(h[4]), int(h[6]) & 0xffffffff
    b.pad = pad
    return b


def _check_tab(b, sizes):
    """raw_tab = the exclusive scan of the delivered records' sizes, closed by the total; the samples = its every EVERY-th entry"""
    want = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    assert b.n == len(sizes), (b.n, len(sizes))
    assert np.array_equal(b.tab[:b.n + 1], want)
    assert np.array_equal(b.smp[:b.ns], [want[min(k * EVERY, b.n)] for k in range(b.ns)])


class _Arena:
    """an arena of `cap` bytes (+ guards) pre-filled with 0xA5, a cursor chain and a raw_start table; piece() appends records
    [lo, hi) of a batch and checks the WHOLE arena against its model"""

    def __init__(self, cap, at=0, pieces=8, records=0):
        import torch
        self.cap = cap
        self.arena = torch.full((cap + 256,), FILL, dtype=torch.uint8, device=DEV)
        self.model = np.full(cap + 256, FILL, dtype=np.uint8)
        self.cursor = torch.full((pieces + 1,), -7, dtype=torch.int64, device=DEV)
        self.cursor[0] = at
        self.start = torch.full((records + 1 + GUARD,), CANARY64, dtype=torch.int64, device=DEV)
        self.k, self.at, self.rec, self.at0 = 0, at, 0, at
        self.starts = []

    def piece(self, b, lo, hi, want, out_cap=None, check=True):
        """want: the bytes of the piece (None: it must be refused - the cursor becomes -1 and nothing is written)"""
        import torch
        cap = self.cap if out_cap is None else out_cap
        N.check(N.lib().rd_bam_raw_gather(N.ptr(b.text), b.src, N.ptr(b.raw_tab), N.ptr(b.summary), lo, hi, len(want) if want is not None else cap,
                                          N.ptr(self.arena), cap, N.C.c_void_p(self.cursor.data_ptr() + 8 * self.k),
                                          N.C.c_void_p(self.cursor.data_ptr() + 8 * (self.k + 1)), N.C.c_void_p(self.start.data_ptr() + 8 * self.rec),
                                          N.stream_ptr(torch.device(DEV))), "rd_bam_raw_gather")
        self.k += 1
        if want is None:
            self.at = -1
        else:
            self.model[self.at:self.at + len(want)] = np.frombuffer(want, np.uint8)
            self.at += len(want)
            self.rec += hi - lo
        if check:
            self.check()

    def check(self):
        import torch
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        if not np.array_equal(got, self.model):
            bad = np.flatnonzero(got != self.model)
            raise AssertionError("arena differs at %d bytes, first %d last %d (piece %d ended at %d)" % (len(bad), bad[0], bad[-1], self.k, self.at))
        cur = self.cursor.cpu().numpy()
        assert int(cur[self.k]) == self.at, (int(cur[self.k]), self.at)
        return got

    def check_starts(self, sizes):
        """raw_start over all pieces so far: continuous, one entry per record and the end"""
        got = self.start.cpu().numpy()
        want = self.at0 + np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == CANARY64).all()


def _rec(name, l_seq, tag_payload, flag=4, rng=None, fill=None):
    rng = rng or np.random.default_rng(l_seq * 64 + tag_payload)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=l_seq))
    payload = bytes(rng.integers(1, 256, tag_payload, dtype=np.uint8)) if fill is None else fill
    return bam.encode_record(dict(name=name, seq=seq, qual=bytes(rng.integers(0, 60, l_seq, dtype=np.uint8)), flag=flag, tags=b"XXZ" + payload + b"\0"))


def _short(i, flag=4):
    """a record of exactly 40 bytes whose bytes depend on i"""
    r = bam.encode_record(dict(name=b"%03d" % (i % 1000), seq=b"", qual=b"", flag=flag))
    assert len(r) == 40
    return r


# ---- alignment ------------------------------------------------------------------------------------------------------------------------
def test_alignment_every_residue():
    recs = [_rec(b"ab"[:1 + t % 2], l, t) for t in range(41) for l in (0, 1, 2, 31, 32, 33)]      # (the name's length: else 12 of the 16 source residues)
    data = b"".join(recs)
    walk = _walk(data)
    assert [s for _, s in walk] == [len(r) for r in recs]
    b = _index(data, 1)
    assert b.status == 0
    _check_tab(b, [s for _, s in walk])
    src_res, dst_res, size_res = {(b.pad + o) % 16 for o, _ in walk}, set(), {s % 16 for _, s in walk}
    n = len(recs)
    for c0 in range(16):
        a = _Arena(len(data) + 64, at=c0, pieces=64, records=n)
        lo, step = 0, 1
        while lo < n:                                # pieces of 1, 2, 3, ... records: launches begin and end at many residues
            hi = min(n, lo + step)
            dst_res.add(a.at % 16)
            a.piece(b, lo, hi, b"".join(recs[lo:hi]), check=False)
            lo, step = hi, step + 1
        got = a.check()
        assert got[c0:c0 + len(data)].tobytes() == data == bam.select(data, range(n), start=0)
        a.check_starts([len(r) for r in recs])
    assert len(src_res) == len(dst_res) == len(size_res) == 16, (src_res, dst_res, size_res)
    # every record alone, at a cursor of every residue: source and destination residues in all combinations that occur
    for k in range(0, n, 5):
        a = _Arena(len(recs[k]) + 32, at=k % 16, pieces=1, records=1)
        a.piece(b, k, k + 1, recs[k])


# ---- gaps -----------------------------------------------------------------------------------------------------------------------------
def test_gaps_between_the_delivered_records():
    rng = np.random.default_rng(3)
    recs = []
    for i in range(300):
        flag = (0x100 if i % 2 else 0x800) if i % 3 == 0 else 4            # (record 0 is skipped)
        recs.append(_rec(b"g%d" % i, int(rng.integers(0, 40)), int(rng.integers(0, 30)), flag=flag, rng=rng))
    recs += [_short(i, flag=0x100) for i in range(S // 40 + 50)]         # a run of skipped records longer than a segment
    recs += [_rec(b"h%d" % i, int(rng.integers(0, 40)), int(rng.integers(0, 30)), rng=rng) for i in range(50)]
    recs.append(_short(7, flag=0x800))                                     # the last record of the window is skipped
    data = b"".join(recs)
    walk = _walk(data)
    all_recs = list(bam.records(data, start=0))
    assert all_recs[0].skipped and all_recs[-1].skipped and 0 < len(walk) < len(recs) - S // 40
    b = _index(data, 1)
    assert b.status == 0
    sizes = [s for _, s in walk]
    _check_tab(b, sizes)
    n = len(walk)
    want = [data[o:o + s] for o, s in walk]
    a = _Arena(sum(sizes) + 16, pieces=3, records=n)
    for lo, hi in ((0, 150), (150, 201), (201, n)):                        # (the long run of skipped records lies inside the second piece)
        a.piece(b, lo, hi, b"".join(want[lo:hi]))
    assert a.check()[:sum(sizes)].tobytes() == bam.select(data, range(n), start=0)
    a.check_starts(sizes)


# ---- record sizes and ranges ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """300 records of 40 bytes, one of 3 S bytes, 300 of 40 bytes: a record over many workgroup trips, a trip over hundreds of records"""
    rng = np.random.default_rng(4)
    body = bytes(rng.integers(1, 256, 3 * S - 36 - 4 - 4, dtype=np.uint8))
    recs = [_short(i) for i in range(300)] + [_rec(b"big", 0, 0, fill=body)] + [_short(i) for i in range(300, 600)]
    assert len(recs[300]) == 3 * S
    data = b"".join(recs)
    b = _index(data, 1)
    assert b.status == 0 and b.n == 601
    _check_tab(b, [len(r) for r in recs])
    return recs, data, b


def _three_pieces(b, recs, lo, hi, cuts, at=0):
    """records [lo, hi) as three chained pieces, the arena checked after each"""
    m1, m2 = sorted(cuts)
    total = sum(len(r) for r in recs[lo:hi])
    a = _Arena(at + total + 48, at=at, pieces=3, records=hi - lo)
    for p, q in ((lo, m1), (m1, m2), (m2, hi)):
        a.piece(b, p, q, b"".join(recs[p:q]))
    assert int(a.cursor.cpu().numpy()[3]) == at + total
    a.check_starts([len(r) for r in recs[lo:hi]])


def test_ranges_as_three_chained_pieces(big):
    recs, data, b = big
    n = len(recs)
    for lo, hi in ((0, 0), (0, 1), (n - 1, n), (300, 301), (0, n)):
        _three_pieces(b, recs, lo, hi, (lo, hi))                           # (an empty piece in front and behind)
        _three_pieces(b, recs, lo, hi, (lo + (hi - lo) // 3, lo + 2 * (hi - lo) // 3), at=9)
    rng = np.random.default_rng(6)
    for _ in range(32):
        lo = int(rng.integers(0, n))
        hi = int(rng.integers(lo, n + 1))
        cuts = (int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)))
        _three_pieces(b, recs, lo, hi, cuts, at=int(rng.integers(0, 40)))
    # a piece boundary inside a 16-byte granule on both sides of the big record
    _three_pieces(b, recs, 290, 310, (300, 301), at=3)


def test_capacity_one_byte_short(big):
    recs, data, b = big
    for lo, mid, hi in ((0, 300, 301), (300, 301, 400), (10, 11, 12)):
        total = sum(len(r) for r in recs[lo:hi])
        a = _Arena(total + 64, pieces=3, records=hi - lo)
        a.piece(b, lo, mid, b"".join(recs[lo:mid]), out_cap=total - 1)    # (fits)
        a.piece(b, mid, hi, None, out_cap=total - 1)                       # one byte short: refused, nothing written
        a.piece(b, hi, hi, None, out_cap=total + 64)                       # the cursor stays -1, even for a piece of nothing
        a = _Arena(total + 64, pieces=1, records=hi - lo)
        a.piece(b, lo, hi, b"".join(recs[lo:hi]), out_cap=total)           # exactly enough
    a = _Arena(len(data) + 64, pieces=1)
    a.piece(b, 0, len(recs) + 1, None)                                     # records behind n_records: refused on the device


# ---- carry ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["block_size", "fixed_fields", "tags"])
def test_a_record_cut_between_two_chained_batches(where):
    rng = np.random.default_rng(8)
    recs = [_rec(b"c%d" % i, int(rng.integers(0, 60)), int(rng.integers(0, 40)), flag=0x100 if i % 5 == 4 else 4, rng=rng) for i in range(80)]
    data = b"".join(recs)
    walk = _walk(data)
    k = 37                                                                 # the delivered record that is cut
    off, size = walk[k]
    cut = off + {"block_size": 2, "fixed_fields": 20, "tags": size - 3}[where]
    b1 = _index(data[:cut], 0)
    assert b1.status == 0 and b1.n == k and b1.consumed - b1.begin == off
    _check_tab(b1, [s for _, s in walk[:k]])
    b2 = _index(data[cut:], 1, prev=b1)
    assert b2.status == 0 and b2.pad - b2.begin == cut - off
    _check_tab(b2, [s for _, s in walk[k:]])
    a = _Arena(size + 32, at=5, pieces=1, records=1)
    a.piece(b2, 0, 1, data[off:off + size])                                # the record gathered from batch 2 is the original
    rest = [data[o:o + s] for o, s in walk]
    a = _Arena(len(data), pieces=2, records=len(walk))
    a.piece(b1, 0, b1.n, b"".join(rest[:k]))                               # one chunk from two batches
    a.piece(b2, 0, b2.n, b"".join(rest[k:]))
    assert a.check()[:a.at].tobytes() == bam.select(data, range(len(walk)), start=0)
    a.check_starts([s for _, s in walk])


# ---- damage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["block=31", "no_nul", "cut_in_record", "cut_in_block_size"])
def test_the_records_in_front_of_the_damage(what):
    rng = np.random.default_rng(9)
    good = [_rec(b"d%d" % i, int(rng.integers(0, 60)), int(rng.integers(0, 40)), flag=0x800 if i % 4 == 1 else 4, rng=rng) for i in range(120)]
    bad = W.G._damaged(what, _rec(b"damaged", 30, 10))
    data = b"".join(good) + bad + (b"" if what.startswith("cut") else b"".join(good[:5]))
    walk = _walk(data)
    assert len(walk) == sum(1 for i in range(120) if i % 4 != 1)
    b = _index(data, 1)
    assert b.status == (N.BAM_TRUNCATED if what.startswith("cut") else N.BAM_RECORD)
    _check_tab(b, [s for _, s in walk])
    want = [data[o:o + s] for o, s in walk]
    a = _Arena(sum(len(w) for w in want) + 16, pieces=2, records=len(want))
    a.piece(b, 0, 40, b"".join(want[:40]))
    a.piece(b, 40, len(want), b"".join(want[40:]))
    a.check_starts([len(w) for w in want])


def test_a_batch_that_is_not_framed():
    recs = [_short(i) for i in range(100)]
    data = b"".join(recs)
    b = _index(data, 1, cap_records=50)                                    # more records than the tables hold: RD_FQ_LINES
    assert b.status == LINES
    assert (b.tab[:b.cap] == CANARY64).all(), "raw_tab written for a batch that is not framed"
    assert (b.smp[:b.ns] == -1).all()
    a = _Arena(4096, pieces=2)
    a.piece(b, 0, 1, None)
    a.piece(b, 0, 0, None)


# ---- binary bytes through the device deflate ------------------------------------------------------------------------------------------------
def test_the_device_deflate_takes_binary_records():
    import torch
    from ribodetector_amd.gz import DeviceGzip, DeviceSelect
    rng = np.random.default_rng(10)
    recs = []
    for i in range(400):
        fill = bytes(range(256)) if i % 50 == 0 else bytes(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8))
        recs.append(bam.encode_record(dict(name=b"z%d" % i, seq="ACGT" * (i % 9), qual=bytes(4 * (i % 9)),
                                           tags=b"MLBC" + struct.pack("<i", len(fill)) + fill)))
    data = b"".join(recs)
    assert set(data) == set(range(256))
    b = _index(data, 1)
    assert b.status == 0 and b.n == 400
    a = _Arena(len(data) + 100, pieces=1, records=400)
    a.piece(b, 0, 400, data)
    labels = torch.from_numpy((np.arange(400) % 3 == 0).astype(np.int8)).to(DEV)
    rs = a.start[:401].contiguous()
    want = b"".join(recs[i] for i in range(400) if i % 3 == 0)
    out, info = DeviceGzip(DEV).compress_selected(a.arena, rs, labels, 1)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert int(info[3]) == 0 and int(info[1]) == len(want)
    comp = out[:int(info[0])].cpu().numpy().tobytes()
    assert gzip.decompress(comp) == want
    out, info = DeviceSelect(DEV).pack_selected(a.arena, rs, labels, 1)
    torch.cuda.synchronize()
    assert out[:int(info.cpu().numpy()[1])].cpu().numpy().tobytes() == want
