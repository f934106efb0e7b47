"""The records of a chunk partitioned by key on the GPU (C ABI rd_group_keys / rd_group_pack / rd_gz_compress_grouped,
csrc/rd_group_pack.hpp) against the plain statement tests/group_truth.py.

rd_group_pack is compared byte for byte. The compressed bytes of rd_gz_compress_grouped are NOT compared with another call's (which
lane of a strip wins a hash bucket is unspecified in the encoder): every key's members must inflate to exactly the statement's bytes,
be ceil(bytes / 65,280) complete BGZF members with a true BC size, CRC-32 and ISIZE, and lie compactly, in key order, in `out`."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_truth as GT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEMBER = 65280


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(recs):
    text = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
    rs = np.zeros(len(recs) + 1, dtype=np.int64)
    rs[1:] = np.cumsum([len(r) for r in recs])
    return text, rs


def _members(comp):
    """[inflated bytes] of the BGZF members of `comp`, each checked: header, BC size <= 65,536, CRC-32, ISIZE <= 65,280"""
    p, out = 0, []
    while p < len(comp):
        assert comp[p:p + 4] == b"\x1f\x8b\x08\x04" and comp[p + 10:p + 16] == b"\x06\x00BC\x02\x00", (p, comp[p:p + 18])
        bsize = struct.unpack("<H", comp[p + 16:p + 18])[0] + 1
        assert bsize <= 65536 and p + bsize <= len(comp)
        body = zlib.decompress(comp[p + 18:p + bsize - 8], -15)
        crc, isize = struct.unpack("<II", comp[p + bsize - 8:p + bsize])
        assert isize == len(body) <= MEMBER and crc == (zlib.crc32(body) & 0xffffffff)
        out.append(body)
        p += bsize
    return out


def _check(recs, keys, K, gs=None):
    """both calls over (recs, keys) against the statement; returns the (out, key_tab, info) of the text call as host values"""
    from ribodetector_amd.gz import DeviceGroupSelect
    gs = gs or DeviceGroupSelect(DEV)
    text, rs = _tables(recs)
    want = GT.partition(text.tobytes(), rs, keys, K)
    t, r, k = _dev(text), _dev(rs), _dev(np.asarray(keys, dtype=np.int32))
    out, tab, info = gs.pack_grouped(t, r, k, K, slot="text")       # (a slot each: the two outputs are compared side by side)
    gout, gtab, ginfo = gs.compress_grouped(t, r, k, K, slot="gz")
    torch.cuda.synchronize()
    out, tab, info = out.cpu().numpy(), tab.cpu().numpy(), info.cpu().tolist()
    offs, need = GT.layout(want)
    assert info == [sum(c for _, c in want), need, 0, 0]
    assert tab.tolist() == [[offs[j], len(want[j][0]), want[j][1], 0] for j in range(K)]
    for j in np.flatnonzero(tab[:, 1]):
        assert out[offs[j]:offs[j] + tab[j, 1]].tobytes() == want[j][0], ("text of key", j)
    gout, gtab, ginfo = gout.cpu().numpy(), gtab.cpu().numpy(), ginfo.cpu().tolist()
    total = sum(len(d) for d, _ in want)
    assert ginfo == [int(gtab[:, 1].sum()), total, int(gtab[:, 3].sum()), 0]
    at = 0
    for j in range(K):
        data, count = want[j]
        assert gtab[j, 0] == at and gtab[j, 2] == count and gtab[j, 3] == -(-len(data) // MEMBER), ("table of key", j, gtab[j].tolist(), at)
        if gtab[j, 1]:
            bodies = _members(gout[at:at + gtab[j, 1]].tobytes())
            assert len(bodies) == gtab[j, 3] and all(len(b) == MEMBER for b in bodies[:-1]) and b"".join(bodies) == data, ("members of key", j)
        else:
            assert not data
        at += int(gtab[j, 1])
    assert at == ginfo[0]
    return out, tab, info


def _fastq(rng, n, lo=30, hi=160):
    recs = []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        seq = bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8))
        recs.append(b"@r%d/1\n%s\n+\n%s\n" % (i, seq, b"F" * L))
    return recs


@pytest.mark.parametrize("n", [0, 1, 2048, 2049, 5000])
def test_sizes_around_a_scan_block(n):
    """one scan block of 256 x 8 records, one past it, several (and several parts of the counting partition from 513 records on)"""
    rng = np.random.default_rng(n)
    recs = _fastq(rng, n)
    for K in (2, 7):
        _check(recs, rng.integers(-1, K, n).astype(np.int32), K)


def test_one_key_is_the_unkeyed_selection():
    """K = 1 with every key 0: the text is what rd_select_pack packs for the same selection, and the members inflate to it"""
    from ribodetector_amd.gz import DeviceSelect
    rng = np.random.default_rng(5)
    recs = _fastq(rng, 3000)
    out, tab, info = _check(recs, np.zeros(3000, dtype=np.int32), 1)
    text, rs = _tables(recs)
    sel, sinfo = DeviceSelect(DEV).pack_selected(_dev(text), _dev(rs), torch.zeros(3000, dtype=torch.int8, device=DEV), 0)
    torch.cuda.synchronize()
    assert int(sinfo[1]) == info[1] == len(text) and sel[:len(text)].cpu().numpy().tobytes() == out[:len(text)].tobytes()


def test_many_keys_few_of_them_used_and_the_last_key():
    rng = np.random.default_rng(6)
    recs = _fastq(rng, 1500)
    K = 3075                                             # 3 classes x (1,024 groups + unassigned): the largest K of a run
    used = np.array([0, 1, 1537, 3073, 3074], dtype=np.int32)
    _check(recs, used[rng.integers(0, 5, 1500)], K)
    _check(recs, np.full(1500, K - 1, dtype=np.int32), K)    # every record in the LAST key
    _check(recs, np.full(1500, -1, dtype=np.int32), 2)       # no record in any key: nothing written, the table all zero
    K = 4097                                             # beyond the keys whose counters a wave keeps in LDS
    _check(recs[:700], np.array([0, 5, 4095, 4096], dtype=np.int32)[rng.integers(0, 4, 700)], K)


def test_the_partition_is_stable():
    """keys drawn over 50 keys with 218-byte records that differ only in their number: any two records of a key swapped would show"""
    rng = np.random.default_rng(7)
    n = 6000
    recs = [b"@%08d\n" % i + b"ACGT" * 26 + b"\n+\n" + b"F" * 100 + b"\n" for i in range(n)]
    assert len(recs[0]) == 218
    _check(recs, rng.integers(0, 50, n).astype(np.int32), 50)


def test_member_boundaries_and_odd_records():
    """keys whose text is exactly 65,279 / 65,280 / 65,281 / 2 x 65,280 bytes; one record of 200,000 bytes that spans four members next
    to short ones; a zero-length record; records of one byte"""
    rng = np.random.default_rng(8)
    queues = []
    for total in (MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER):
        body = bytes(rng.choice(list(b"ACGTN\n"), total).astype(np.uint8))
        queues.append([body[i:i + 997] for i in range(0, total, 997)])
    recs, keys = [], []
    while any(queues):                                   # the four keys' records interleaved, each key's in their order
        key = int(rng.choice([k for k in range(4) if queues[k]]))
        recs.append(queues[key].pop(0))
        keys.append(key)
    _check(recs, keys, 4)
    big = bytes(rng.choice(list(b"ACGT"), 200000).astype(np.uint8))
    recs = [b"ab\n", big, b"", b"x", b"y", b"", b"cd\n", b"z"]
    _check(recs, [1, 0, 0, 1, 2, 2, 0, 1], 3)
    _check([b"q"] * 3000, rng.integers(-1, 3, 3000).astype(np.int32), 3)


def test_binary_records_as_source():
    """raw (binary) records, as --bam_output selects them: every byte value, lengths that are no multiple of anything"""
    rng = np.random.default_rng(9)
    recs = [bytes(rng.integers(0, 256, int(rng.integers(36, 400)), dtype=np.uint8)) for _ in range(2500)]
    _check(recs, rng.integers(-1, 9, 2500).astype(np.int32), 9)


@pytest.mark.parametrize("n", [0, 1, 257, 3000])
def test_keys_word_for_word(n):
    """rd_group_keys against group_truth.keys: a key per unit, the interleaved expansion with stride 2 for both mates, a class that
    is not written, and the flags for a label / a row outside its range"""
    from ribodetector_amd.gz import DeviceGroupSelect
    gs = DeviceGroupSelect(DEV)
    rng = np.random.default_rng(n)
    G = 3
    rows = rng.integers(0, G + 3, 2 * n + 2).astype(np.int32)
    labels = rng.integers(-1, 2, n).astype(np.int8)
    for slots in ([0, 1, 2], [-1, 0, -1], [-1, -1, 0], [1, -1, 0]):
        for first, stride, mate in ((0, 1, -1), (0, 2, -1), (0, 2, 0), (0, 2, 1), (1, 2, -1)):
            got, info = gs.keys(_dev(rows), _dev(labels), slots, G, first, stride, mate)
            torch.cuda.synchronize()
            want, flags = GT.keys(rows, labels, slots, G, first, stride, mate)
            assert got.cpu().tolist() == want and info.cpu().tolist() == [flags, n, 0, 0] and flags == 0
    if n:
        for bad_rows, bad_labels, flag in ((G + 3, None, 2), (-1, None, 2), (None, 2, 1), (None, -2, 1), (G + 3, 2, 3)):
            r2, l2 = rows.copy(), labels.copy()
            if bad_rows is not None:
                r2[n // 2] = bad_rows
            if bad_labels is not None:
                l2[n - 1] = bad_labels
            got, info = gs.keys(_dev(r2), _dev(l2), [0, 1, 2], G)
            torch.cuda.synchronize()
            want, flags = GT.keys(r2, l2, [0, 1, 2], G)
            assert flags == flag and info.cpu().tolist() == [flag, n, 0, 0] and got.cpu().tolist() == want


def test_faults_are_reported_not_taken():
    """a key equal to K, a key of -2, out_cap one byte short (info[1] says what was needed), a record table that describes more bytes
    than the text has, a workspace one byte short, a misaligned out: each one an answer in info or a refusal on the host"""
    from ribodetector_amd import _native as N
    L = N.lib()
    rng = np.random.default_rng(11)
    recs = _fastq(rng, 1200)
    text, rs = _tables(recs)
    K, n, tb = 4, len(recs), len(text)
    keys = rng.integers(-1, K, n).astype(np.int32)
    want = GT.partition(text.tobytes(), rs, keys, K)
    _, need = GT.layout(want)
    t, r = _dev(text), _dev(rs)
    ws = torch.empty(int(L.rd_group_workspace_bytes(n, tb, K, 1)), dtype=torch.uint8, device=DEV)
    out = torch.zeros(int(L.rd_gz_grouped_out_bound(tb, K)) + 512, dtype=torch.uint8, device=DEV)
    tab = torch.empty((K, 4), dtype=torch.int64, device=DEV)
    info = torch.empty(4, dtype=torch.int64, device=DEV)

    def call(fn, keys=keys, r=r, tb=tb, out=out, cap=None, ws_bytes=None):
        k = _dev(keys)
        rc = getattr(L, fn)(N.ptr(t), tb, N.ptr(r), N.ptr(k), n, K, out.data_ptr(), out.numel() if cap is None else cap, N.ptr(tab), N.ptr(info),
                            N.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, N.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc, info.cpu().tolist(), tab.cpu().numpy()

    for fn, gz in (("rd_group_pack", 0), ("rd_gz_compress_grouped", 1)):
        for bad in (K, -2):
            k2 = keys.copy()
            k2[777] = bad
            rc, inf, tb_ = call(fn, keys=k2)
            assert rc == 0 and inf == [0, 0, 0, 1] and not tb_.any(), (fn, bad, inf)
        r2 = rs.copy()
        r2[-1] = tb + 1                                      # the last record runs past the text
        k2 = keys.copy()
        k2[-1] = 0
        rc, inf, tb_ = call(fn, keys=k2, r=_dev(r2))
        assert rc == 0 and inf == [0, 0, 0, 2] and not tb_.any()
        r2 = rs.copy()
        r2[500] = rs[501] + 5                                # a descending entry: record 500 would have a negative length
        k2[500] = 0
        rc, inf, tb_ = call(fn, keys=k2, r=_dev(r2))
        assert rc == 0 and inf == [0, 0, 0, 2] and not tb_.any()
        rc, inf, _ = call(fn, ws_bytes=int(L.rd_group_workspace_bytes(n, tb, K, gz)) - 1)
        assert rc == -4 and L.rd_last_error().startswith(fn.encode() + b": workspace too small")
        rc, inf, _ = call(fn, out=out[1:])
        assert rc == -1 and b"aligned" in L.rd_last_error()
    rc, inf, tb_ = call("rd_group_pack", cap=need - 1)
    assert rc == 0 and inf[1] == need and inf[3] == 4
    rc, inf, tb_ = call("rd_group_pack", cap=need)
    assert rc == 0 and inf[1] == need and inf[3] == 0
    rc, inf, tb_ = call("rd_gz_compress_grouped")
    assert rc == 0 and inf[3] == 0
    rc, inf, tb_ = call("rd_gz_compress_grouped", cap=1024)      # (the compressed size is not the same from call to call: far too small)
    assert rc == 0 and inf[0] > 1024 and inf[3] == 4


@pytest.mark.parametrize("n,chosen", [(1024, list(range(300, 311)) + [1023]), (257, [256])])
def test_workgroups_of_the_pack_with_nothing_to_write(n, chosen):
    """whole blocks of 256 records of which none is selected (a workgroup of the selection pack whose output range is empty, workgroups
    of the grouped pack behind the last place), a last block that holds one place; records of 0 .. 40 bytes, so that most pieces of
    16 bytes span several records. Labels 1 (a few records), 5 (none) and 0 (all the others), through all four entry points."""
    from ribodetector_amd.gz import DeviceGroupSelect, DeviceGzip, DeviceSelect
    rng = np.random.default_rng(n)
    recs = [bytes(rng.integers(33, 127, int(L), dtype=np.uint8)) for L in rng.integers(0, 41, n)]
    assert min(map(len, recs)) == 0 and any(0 < len(r) < 16 for r in recs)
    text, rs = _tables(recs)
    labels = np.zeros(n, dtype=np.int8)
    labels[chosen] = 1
    t, r, lab = _dev(text), _dev(rs), _dev(labels)
    sel, gz, gs = DeviceSelect(DEV), DeviceGzip(DEV), DeviceGroupSelect(DEV)
    for label in (1, 5, 0):
        picked = np.flatnonzero(labels == label)
        want = b"".join(recs[i] for i in picked)
        members = -(-len(want) // MEMBER)
        out, info = sel.pack_selected(t, r, lab, label)
        gout, ginfo = gz.compress_selected(t, r, lab, label)
        keys = _dev(np.where(labels == label, 0, -1).astype(np.int32))
        kout, ktab, kinfo = gs.pack_grouped(t, r, keys, 1, slot="text")
        zout, ztab, zinfo = gs.compress_grouped(t, r, keys, 1, slot="gz")
        torch.cuda.synchronize()
        info = info.cpu().tolist()
        assert (info[1], info[3]) == (len(want), 0) and out[:len(want)].cpu().numpy().tobytes() == want, (label, info)
        ginfo = ginfo.cpu().tolist()
        assert ginfo[1:] == [len(want), members, 0], (label, ginfo)
        bodies = _members(gout[:ginfo[0]].cpu().numpy().tobytes())
        assert len(bodies) == members and b"".join(bodies) == want, label
        assert ktab.cpu().tolist() == [[0, len(want), len(picked), 0]] and kinfo.cpu().tolist() == [len(picked), len(want), 0, 0], label
        assert kout[:len(want)].cpu().numpy().tobytes() == want, label
        ztab, zinfo = ztab.cpu().tolist(), zinfo.cpu().tolist()
        assert ztab == [[0, zinfo[0], len(picked), members]] and zinfo[1:] == [len(want), members, 0], (label, ztab, zinfo)
        bodies = _members(zout[:zinfo[0]].cpu().numpy().tobytes())
        assert len(bodies) == members and b"".join(bodies) == want, label
