"""The tag walk, the group rows and the per-group counters on the GPU (C ABI rd_bam_tag_find / rd_bam_group_rows /
rd_bam_group_accumulate, csrc/rd_bam_tags.hpp) against the rule in bam.py and a numpy restatement. The raw views are records of
bam.encode_record laid out back to back; every lane mapping of the find kernel (RD_TAG_LANES) sees every case."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LANES = [None, "4", "16"]                    # lanes per record of the find kernel; None: the mapping the library chooses


@pytest.fixture
def lanes(monkeypatch):
    def use(v):
        if v is None:
            monkeypatch.delenv("RD_TAG_LANES", raising=False)
        else:
            monkeypatch.setenv("RD_TAG_LANES", v)
    return use


def _dev(raw, starts):
    import torch
    pad = np.frombuffer(raw + b"\xa5" * 64, dtype=np.uint8).copy()         # (bytes behind the view that are no NUL: the tensor is longer than the view)
    return torch.from_numpy(pad).to(DEV)[:len(raw)], torch.tensor(starts, dtype=torch.int64, device=DEV)


def _find(recs, tag=T.TARGET):
    from ribodetector_amd import groups
    raw, st = T.view(recs)
    d_raw, d_st = _dev(raw, st)
    vo, vl, vt = groups.tag_find(d_raw, d_st, len(recs), tag)
    got = list(zip(vo.cpu().tolist(), vl.cpu().tolist(), vt.cpu().tolist()))
    return raw, st, got, (d_raw, d_st, vo, vl, vt)


# ---- find -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", LANES)
def test_find_on_the_hand_built_cases(lanes, mapping):
    lanes(mapping)
    recs = [c[1] for c in T.CASES]
    raw, st, got, _ = _find(recs)
    want = T.reference(raw, st)
    for k, (name, _, says) in enumerate(T.CASES):
        assert got[k] == want[k], (name, got[k], want[k])
        assert T.check_case(raw, st[k], st[k + 1], got[k], says), (name, got[k], says)
    # another tag over the same view: general over tags and types
    for tag in (b"NM", b"ML", b"MM", b"XH"):
        raw, st, got, _ = _find(recs, tag)
        assert got == T.reference(raw, st, tag), tag


@pytest.mark.parametrize("mapping", LANES)
@pytest.mark.parametrize("n_rec", [1, 63, 64, 65, 257])
def test_find_record_counts_around_the_wave_and_the_workgroup(lanes, mapping, n_rec):
    lanes(mapping)
    base = [c[1] for c in T.CASES]
    recs = [base[(5 * k + n_rec) % len(base)] for k in range(n_rec)]
    raw, st, got, _ = _find(recs)
    assert got == T.reference(raw, st)


@pytest.mark.parametrize("mapping", LANES)
def test_find_seeded_sweep(lanes, mapping):
    lanes(mapping)
    recs = T.random_records(7, 300)
    raw, st, got, _ = _find(recs)
    want = T.reference(raw, st)
    assert got == want
    assert min(sum(1 for w in want if w[0] == v) for v in (-1, -2)) >= 15 and sum(1 for w in want if w[0] >= 0) >= 100


def test_find_a_view_that_is_no_view(lanes):
    """raw_start entries that run backwards, leave the buffer or leave less than a record's fixed part: malformed, nothing is read"""
    import torch
    from ribodetector_amd import groups
    lanes(None)
    r = T.rec(T.Z(b"RG", b"a"))
    raw = torch.from_numpy(np.frombuffer(r * 3, dtype=np.uint8).copy()).to(DEV)
    n = len(r)
    st = torch.tensor([0, n, n - 1, 2 * n, 1 << 40, 2 * n + 20, 3 * n], dtype=torch.int64, device=DEV)
    vo, vl, vt = groups.tag_find(raw, st, 6, b"RG")
    assert vo.cpu().tolist()[0] >= 0 and vo.cpu().tolist()[1:] == [-2] * 5 and vl.cpu().tolist()[1:] == [0] * 5 and vt.cpu().tolist()[1:] == [0] * 5
    vo, vl, vt = groups.tag_find(raw, st, 0, b"RG")
    assert vo.numel() == 0


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def _rows_case(ids, values):
    """records with RG:Z:<value> (None: no RG; an int: RG:i) -> (device rows, the rule's rows over the SORTED ids)"""
    from ribodetector_amd import groups
    recs = []
    for k, v in enumerate(values):
        tags = T.scalar(b"NM", "i", k)
        if isinstance(v, int):
            tags += T.scalar(b"RG", "i", v)
        elif v is not None:
            tags += T.Z(b"RG", v)
        recs.append(T.rec(tags, name=b"r%d" % k))
    recs.append(T.rec(T.scalar(b"NM", "i", 1) + b"RG"))                      # malformed
    raw, st, got, (d_raw, d_st, vo, vl, vt) = _find(recs)
    d = groups.Dictionary(DEV, ids)
    rows = d.rows(d_raw, vo, vl, vt).cpu().tolist()
    want = [bam.group_row(raw, *g, d.sorted) for g in T.reference(raw, st)]
    return rows, want, d


@pytest.mark.parametrize("G", [1, 2, 3, 384, 1024, 1025])
def test_rows_of_every_declared_id(G):
    """(up to 1,024 ids the dictionary is searched in LDS, beyond that in global memory)"""
    rng = np.random.default_rng(G)
    ids = sorted({bytes(rng.integers(33, 127, int(rng.integers(1, 12)), dtype=np.uint8)) for _ in range(4 * G)})[:G]
    assert len(ids) == G
    ids = [ids[j] for j in rng.permutation(G)]                               # (header order is not sorted order)
    values = list(ids) + [None, b"", b"~~~~~~~~~~~~~~~~~~~~", 7, ids[0] + b"x", ids[-1][:-1]]
    rows, want, d = _rows_case(ids, values)
    assert rows == want
    assert sorted(rows[:G]) == list(range(G)) and rows[G] == G and rows[G + 3] == G + 2 and rows[-1] == G + 2
    assert [d.sorted[r] for r in rows[:G]] == ids


def test_rows_prefixes_lengths_and_high_bytes():
    ids = [b"abc", b"a", b"ab", b"\xe9", b"\x7f", b"\x80z", b"b"]
    values = ids + [b"", b"abcd", b"abcdefghijklmnopqrstuvwxyz" * 8, b"aa", b"\xe9\x01", b"\x80", b"\xff", None, 3, b"A"]
    rows, want, d = _rows_case(ids, values)
    G = len(ids)
    assert rows == want
    assert d.sorted == [b"a", b"ab", b"abc", b"b", b"\x7f", b"\x80z", b"\xe9"]               # unsigned: 0x80 and 0xe9 behind 0x7f
    assert rows[:G] == [2, 0, 1, 6, 4, 5, 3]
    assert rows[G:] == [G + 1] * 7 + [G, G + 2, G + 1, G + 2]


@pytest.mark.parametrize("pad", [0, 1100])
def test_rows_ids_that_agree_in_their_first_16_bytes(pad):
    """the LDS search compares 16 bytes at a time and must go on behind them; pad: more ids, the search in global memory"""
    stem = b"barcode-kit-0123"
    assert len(stem) == 16
    ids = [stem, stem + b"4", stem + b"45", stem + b"5", stem[:15], stem[:8], stem + b"\xe9", stem + b"4" * 40] + [b"pad%05d" % k for k in range(pad)]
    values = ids[:8] + [stem + b"44", stem + b"3", stem + b"\x80", stem + b"4" * 39, stem + b"4" * 41, stem[:9], None]
    rows, want, d = _rows_case(ids, values)
    G = len(ids)
    assert rows == want and [d.sorted[r] for r in rows[:8]] == ids[:8]
    assert rows[8:] == [G + 1] * 6 + [G, G + 2]


def test_rows_without_declared_groups():
    rows, want, _ = _rows_case([], [b"a", None, 5])
    assert rows == want == [1, 0, 2, 2]


# ---- accumulate -----------------------------------------------------------------------------------------------------------------------
def _stub(l_seq):
    """36 bytes that are a record's fixed part and nothing else: the accumulate pass reads l_seq alone"""
    return struct.pack("<iiiBBHHHIiii", 32, -1, -1, 1, 0, 4680, 0, 4, l_seq, -1, -1, 0)


def _numpy_acc(G, labels, lens_a, rows_a, lens_b=None, rows_b=None):
    acc = np.zeros((G + 3) * 6 + 1, dtype=np.int64)
    for u, lab in enumerate(labels):
        at = (int(rows_a[u]) * 3 + int(lab) + 1) * 2
        acc[at] += 1
        acc[at + 1] += int(lens_a[u]) + (int(lens_b[u]) if lens_b is not None else 0)
        if rows_b is not None and rows_b[u] != rows_a[u]:
            acc[-1] += 1
    return acc


def _view(lens, rows, first=0, stride=1):
    import torch
    raw, st = T.view([_stub(int(x)) for x in lens])
    d_raw, d_st = _dev(raw, st)
    return (d_raw, d_st, torch.tensor(np.asarray(rows, dtype=np.int32), device=DEV), first, stride)


def _acc(G, labels, a, b=None, acc=None):
    import torch
    from ribodetector_amd import groups
    if acc is None:
        acc = torch.zeros(groups.acc_words(G), dtype=torch.int64, device=DEV)
    info = groups.accumulate(acc, G, torch.tensor(np.asarray(labels, dtype=np.int8), device=DEV), a, b)
    return acc, info.cpu().tolist()


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_accumulate_small(n):
    rng = np.random.default_rng(n)
    G = 3
    labels, rows, lens = rng.integers(-1, 2, n), rng.integers(0, G + 3, n), rng.integers(0, 400, n)
    acc, info = _acc(G, labels, _view(list(lens) + [9], list(rows) + [0]))
    assert info[0] == 0 and info[1] == n
    assert np.array_equal(acc.cpu().numpy(), _numpy_acc(G, labels, lens, rows))


def test_accumulate_70000_units_in_one_group_and_two_calls_add():
    """past 65,536 units in one bin: the workgroups' counts and the 64-bit adds are exact; a second call adds to the first"""
    n, G = 70000, 1
    rng = np.random.default_rng(1)
    lens = rng.integers(50, 151, n)
    labels = np.ones(n, dtype=np.int8)
    v = _view(lens, np.zeros(n))
    acc, info = _acc(G, labels, v)
    want = _numpy_acc(G, labels, lens, np.zeros(n, dtype=np.int64))
    assert info[:2] == [0, n] and np.array_equal(acc.cpu().numpy(), want) and want[4] == n
    labels2 = rng.integers(-1, 2, n)
    acc, info = _acc(G, labels2, v, acc=acc)
    assert np.array_equal(acc.cpu().numpy(), want + _numpy_acc(G, labels2, lens, np.zeros(n, dtype=np.int64)))


@pytest.mark.parametrize("G", [384, 700])
def test_accumulate_many_groups_hit_uniformly(G):
    """384 groups: the workgroup's LDS bins; 700: more keys than they hold - the adds go to the accumulator directly"""
    n = 20000
    rng = np.random.default_rng(G)
    labels, rows, lens = rng.integers(-1, 2, n), rng.integers(0, G + 3, n), rng.integers(0, 300, n)
    acc, info = _acc(G, labels, _view(lens, rows))
    assert info[:2] == [0, n] and np.array_equal(acc.cpu().numpy(), _numpy_acc(G, labels, lens, rows))
    assert (acc.cpu().numpy()[:-1].reshape(G + 3, 3, 2)[:, :, 0].sum(1) > 0).all()


def test_accumulate_interleaved_and_two_files():
    import torch
    n, G = 1500, 4
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, 2, n)
    # --interleaved: one view, unit u = records 2 u and 2 u + 1
    lens, rows = rng.integers(0, 300, 2 * n), rng.integers(0, G + 3, 2 * n)
    rows[1::2] = np.where(rng.random(n) < 0.8, rows[0::2], rows[1::2])
    raw, st, rw, _, _ = _view(lens, rows)
    acc, info = _acc(G, labels, (raw, st, rw, 0, 2), (raw, st, rw, 1, 2))
    want = _numpy_acc(G, labels, lens[0::2], rows[0::2], lens[1::2], rows[1::2])
    assert info[:2] == [0, n] and np.array_equal(acc.cpu().numpy(), want) and 0 < want[-1] < n
    # two files: the mates' own views and rows
    la, lb, ra = rng.integers(0, 300, n), rng.integers(0, 300, n), rng.integers(0, G + 3, n)
    rb = np.where(rng.random(n) < 0.5, ra, rng.integers(0, G + 3, n))
    acc, info = _acc(G, labels, _view(la, ra), _view(lb, rb))
    want = _numpy_acc(G, labels, la, ra, lb, rb)
    assert info[:2] == [0, n] and np.array_equal(acc.cpu().numpy(), want) and want[-1] == int((ra != rb).sum()) > 0
    assert torch.cuda.is_available()


def test_accumulate_l_seq_of_2_to_the_31_minus_1():
    """stubs whose l_seq is 2^31 - 1: only l_seq is read, and a bin's bases pass 2^32 (and 2^33 for pairs)"""
    big = (1 << 31) - 1
    n, G = 5, 1
    labels = [1, 1, 1, 0, -1]
    acc, info = _acc(G, labels, _view([big] * n, [0] * n), _view([big] * n, [0, 0, 1, 0, 0]))
    a = acc.cpu().numpy()
    assert info[:2] == [0, n] and np.array_equal(a, _numpy_acc(G, labels, [big] * n, [0] * n, [big] * n, [0, 0, 1, 0, 0]))
    assert a[5] == 6 * big > 1 << 33 and a[-1] == 1


def test_accumulate_refuses_a_bad_label_or_row():
    import torch
    from ribodetector_amd import groups
    G, n = 2, 300
    rng = np.random.default_rng(4)
    labels, rows, lens = rng.integers(-1, 2, n), rng.integers(0, G + 3, n), rng.integers(0, 300, n)
    acc = torch.full((groups.acc_words(G),), 5, dtype=torch.int64, device=DEV)
    for what, bit in (("label", 1), ("row", 2), ("row_neg", 2), ("row_b", 2)):
        lab, ra, rb = labels.copy(), rows.copy(), rows.copy()
        if what == "label":
            lab[170] = 2
        elif what == "row":
            ra[299] = G + 3
        elif what == "row_neg":
            ra[0] = -1
        else:
            rb[64] = G + 3
        _, info = _acc(G, lab, _view(lens, ra), _view(lens, rb), acc=acc)
        assert info[0] == bit, what
        assert (acc.cpu().numpy() == 5).all(), what
    _, info = _acc(G, labels, _view(lens, rows), acc=acc)
    assert info[:2] == [0, n] and np.array_equal(acc.cpu().numpy() - 5, _numpy_acc(G, labels, lens, rows))


def test_device_groups_over_chunks():
    """groups.DeviceGroups.add: find, rows and accumulate over objects that carry a raw view like a reader's chunk"""
    from ribodetector_amd import groups
    header = bam.encode_header(text=b"@RG\tID:zz\tSM:one\n@RG\tID:aa\tSM:two\n@RG\tID:unused\n")
    ids = [b"zz", b"aa", b"unused"]
    rng = np.random.default_rng(5)
    n = 400

    def mate(seed):
        r = np.random.default_rng(seed)
        recs, rows = [], []
        for k in range(n):
            kind = int(r.integers(0, 6))
            tags = T.scalar(b"NM", "i", k) + [T.Z(b"RG", b"zz"), T.Z(b"RG", b"aa"), b"", T.Z(b"RG", b"other"), T.scalar(b"RG", "i", 1), T.Z(b"RG", b"zz")][kind]
            recs.append(T.rec(tags, seq="ACGT" * int(r.integers(0, 30))))
            rows.append([0, 1, 3, 4, 5, 0][kind])                            # header order: zz 0, aa 1, unused 2; none 3, undeclared 4, malformed 5
        return recs, rows

    class Chunk:
        def __init__(self, recs):
            self.raw = _dev(*T.view(recs))

    import torch
    labels = rng.integers(-1, 2, n)
    d_labels = torch.tensor(labels.astype(np.int8), device=DEV)
    (ra, rows_a), (rb, rows_b) = mate(10), mate(11)
    lens = [[struct.unpack_from("<I", x, 20)[0] for x in recs] for recs in (ra, rb)]

    def expect(doc, rows1, lens1, rows2=None, lens2=None):
        per = {}
        for u in range(n):
            c = ("unclassified", "nonrRNA", "rRNA")[labels[u] + 1]
            e = per.setdefault(rows1[u], {"units": {}, "bases": {}})
            e["units"][c] = e["units"].get(c, 0) + 1
            e["bases"][c] = e["bases"].get(c, 0) + lens1[u] + (lens2[u] if lens2 else 0)
        entries = doc["groups"] + [doc["none"], doc["undeclared"], doc["malformed_tags"]]
        for j, e in enumerate(entries):
            for what in ("units", "bases"):
                for c in ("unclassified", "nonrRNA", "rRNA"):
                    assert e[what][c] == per.get(j, {what: {}})[what].get(c, 0), (j, what, c)
        if rows2 is not None:
            assert doc["mate2_differs"] == sum(1 for u in range(n) if rows1[u] != rows2[u]) > 0
    # single-end, in two chunks
    g = groups.DeviceGroups(DEV, header)
    assert [x[0] for x in g.groups] == ids and g.G == 3
    assert g.add([Chunk(ra[:150])], d_labels[:150].contiguous()).cpu().tolist()[0] == 0
    assert g.add([Chunk(ra[150:])], d_labels[150:].contiguous()).cpu().tolist()[:2] == [0, 250]
    doc = groups.to_json(g.result(), g.groups, False, input="a.bam")
    expect(doc, rows_a, lens[0])
    assert [e["id"] for e in doc["groups"]] == ["zz", "aa", "unused"] and doc["groups"][2]["units"]["total"] == 0
    assert groups.units_per_class(g.result(), 3) == [int((labels == v).sum()) for v in (-1, 0, 1)]
    # two files
    g = groups.DeviceGroups(DEV, header)
    assert g.add([Chunk(ra), Chunk(rb)], d_labels).cpu().tolist()[:2] == [0, n]
    expect(groups.to_json(g.result(), g.groups, True), rows_a, lens[0], rows_b, lens[1])
    # interleaved
    g = groups.DeviceGroups(DEV, header)
    il = [x for pair in zip(ra, rb) for x in pair]
    assert g.add([Chunk(il)], d_labels, interleaved=True).cpu().tolist()[:2] == [0, n]
    expect(groups.to_json(g.result(), g.groups, True), rows_a, lens[0], rows_b, lens[1])
