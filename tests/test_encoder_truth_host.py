"""tests/encoder_truth.py against the existing authorities - the CPU oracle (oracle/rd_oracle.c), the golden fixtures (the
reference's own output) and torch on the CPU - so that a wrong numpy reference cannot agree with a wrong kernel in
tests/test_gpu_encoders.py and tests/test_gpu_labels.py. No GPU. Everything is exact equality."""
import itertools

import numpy as np
import pytest

import encoder_truth as ET

MODES = ("none", "rrna", "norrna", "both")
# the bytes of the test arenas: all 256 values, A C G T U three times as often as the rest together
BYTE_TABLE = np.concatenate([np.arange(256, dtype=np.uint8), np.frombuffer(b"ACGTU" * 154, dtype=np.uint8)[:768]])


def ragged_batch(n, max_len, seed, lo=0, slot=None):
    """n reads of lo...2*max_len bases over all 256 byte values, read i starting at an arena offset that is i mod 16, so that
    every alignment of a read occurs; returns (arena uint8, off int64[n], lens int32[n])"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, 2 * max_len + 1, size=n).astype(np.int32)
    return place_reads(lens, rng, slot)


def place_reads(lens, rng, slot=None):
    lens = np.asarray(lens, dtype=np.int32)
    n = len(lens)
    room = np.maximum(lens, 0).astype(np.int64)
    if slot is None:                               # packed: the next multiple of 16 past the previous read, plus i mod 16
        off = np.zeros(n, dtype=np.int64)
        end = 0
        for i in range(n):
            off[i] = (end + 15) // 16 * 16 + i % 16
            end = off[i] + room[i]
    else:                                          # one slot per read (vectorised, for the large batches)
        assert slot % 16 == 0 and slot >= int(room.max(initial=0)) + 16
        off = np.arange(n, dtype=np.int64) * slot + np.arange(n, dtype=np.int64) % 16
        end = n * slot
    arena = BYTE_TABLE[rng.integers(0, len(BYTE_TABLE), size=int(end) + 16, dtype=np.uint16)]
    k = min(256, len(arena))
    arena[:k] = np.arange(k, dtype=np.uint8)       # every byte value is there, inside the first reads
    return arena, off, lens


def special_values():
    return np.array([-np.inf, -1.0, -0.0, 0.0, 2.0 ** -140, 1.0, 1.0 + 2.0 ** -23, 2.0 ** 24, 2.0 ** 24 + 2.0, np.inf, np.nan],
                    dtype=np.float32)


def special_table():
    """(l1, l2) float32 [11^4, 2]: every combination of the special logits in the four slots (x1, y1, x2, y2)"""
    v = special_values()
    assert v[4] > 0 and v[4] < np.finfo(np.float32).tiny and v[6] > 1 and v[8] - v[7] == 2     # a denormal; 1 + ulp; exact in fp32
    combos = np.array(list(itertools.product(range(len(v)), repeat=4)))
    t = v[combos]
    return np.ascontiguousarray(t[:, 0:2]), np.ascontiguousarray(t[:, 2:4])


def tied_logits(n, seed):
    """random float32 logits [n, 2] x 2 with about 5 % exact ties planted: within mate 1, within mate 2, and of the two sums"""
    rng = np.random.default_rng(seed)
    l1 = rng.standard_normal((n, 2)).astype(np.float32) * 3
    l2 = rng.standard_normal((n, 2)).astype(np.float32) * 3
    kind = rng.integers(0, 60, size=n)
    l1[kind == 0, 1] = l1[kind == 0, 0]
    l2[kind == 1, 1] = l2[kind == 1, 0]
    l2[kind == 2, 0], l2[kind == 2, 1] = l1[kind == 2, 1], l1[kind == 2, 0]      # x1 + x2 == y1 + y2 exactly (addition commutes)
    return l1, l2


@pytest.fixture(scope="module")
def batch():
    arena, off, lens = ragged_batch(400, 37, seed=3)
    lens[::17] = 0                                                               # empty reads
    return arena, off, lens


def test_tables_cover_what_they_claim(batch):
    arena, off, lens = batch
    assert set(arena.tolist()) == set(range(256)) and set((off % 16).tolist()) == set(range(16))
    assert (lens == 0).sum() > 10 and lens.max() > 37 * 2 - 5
    for ch in range(256):
        assert ET.LUT[ch] == {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}.get(ch, 4)
    assert set(np.frombuffer(b"acgtuN", dtype=np.uint8).tolist()) <= set(np.flatnonzero(ET.LUT == 4).tolist())


@pytest.mark.parametrize("max_len,stride", [(37, 37), (37, 40), (1, 1), (16, 20), (100, 101)])
def test_codes_and_padded_match_the_oracle(oracle, batch, max_len, stride):
    arena, off, lens = batch
    c = ET.codes(arena, off, lens, max_len, stride)
    p = ET.padded(arena, off, lens, max_len)
    assert c.shape == (len(lens), stride) and c.dtype == np.uint8 and p.shape == (len(lens), max_len, 4) and p.dtype == np.float32
    for i in range(len(lens)):
        s = bytes(arena[off[i]:off[i] + lens[i]])
        want = np.full(stride, 4, dtype=np.uint8)
        want[:min(len(s), max_len)] = oracle.encode_codes(s[:max_len])
        assert (c[i] == want).all(), i
        assert (p[i] == oracle.encode_padded(s, max_len)).all(), i


@pytest.mark.parametrize("max_len", [1, 2, 37, 50, 74, 200])
def test_pack_matches_the_oracle(oracle, batch, max_len):
    arena, off, lens = batch
    data, bs, si, ui = oracle.pack_sequence(arena, off, lens, max_len)
    order, inverse, sizes, total = ET.pack_plan(lens, max_len)
    assert (order == si).all() and (inverse == ui).all() and total == len(data)
    assert sizes.shape == (max_len,) and (sizes[:len(bs)] == bs).all() and (sizes[len(bs):] == 0).all()
    got = ET.pack_data(arena, off, lens, max_len)
    assert got.dtype == np.float32 and got.shape == data.shape and (got == data).all()
    T = ET.steps(lens, max_len)
    assert (sizes == [(T > t).sum() for t in range(max_len)]).all() and total == T.sum()


def test_pack_plan_clamps_negative_lengths():
    lens = np.array([3, -1, 0, 9, -2147483648, 2, 2147483647, 3], dtype=np.int32)      # (the oracle does not define these: by hand)
    order, inverse, sizes, total = ET.pack_plan(lens, 5)
    assert order.tolist() == [3, 6, 0, 7, 5, 1, 2, 4] and inverse[order].tolist() == list(range(8))
    assert sizes.tolist() == [5, 5, 4, 2, 2] and total == 18


def test_fixtures(golden):
    d = golden.npz("collate")
    L = int(d["max_len"])
    off, lens = d["offsets"][:-1], d["lens"]
    assert (ET.padded(d["arena"], off, lens, L) == d["padded"]).all()
    order, inverse, sizes, total = ET.pack_plan(lens, L)
    assert (sizes == d["batch_sizes"]).all() and total == len(d["data"])
    assert (ET.steps(lens, L)[order] == ET.steps(lens, L)[d["sorted_indices"]]).all() and (order[inverse] == np.arange(len(lens))).all()
    assert (ET.pack_data(d["arena"], off, lens, L) == d["data"]).all()
    p = golden.npz("pe")
    for mode in MODES:
        assert (ET.pair_fuse(p["r1_logits"], p["r2_logits"], mode) == p["labels_" + mode]).all(), mode


def test_pack_matches_torch():
    import torch
    from torch.nn.utils.rnn import PackedSequence, pack_sequence, pad_packed_sequence
    arena, off, lens = ragged_batch(300, 20, seed=8, lo=1)
    for max_len in (1, 13, 20, 45):
        T = ET.steps(lens, max_len)
        onehots = [torch.from_numpy(ET.ONEHOT[ET.LUT[arena[off[i]:off[i] + T[i]]]]) for i in range(len(lens))]
        want = pack_sequence(onehots, enforce_sorted=False)
        order, inverse, sizes, total = ET.pack_plan(lens, max_len)
        tmax = int(T.max())
        assert (sizes[:tmax] == want.batch_sizes.numpy()).all() and (sizes[tmax:] == 0).all() and total == want.data.shape[0]
        want_pad = pad_packed_sequence(want, batch_first=True)[0]
        mine = PackedSequence(torch.from_numpy(ET.pack_data(arena, off, lens, max_len)), torch.from_numpy(sizes[:tmax]),
                              torch.from_numpy(order), torch.from_numpy(inverse))
        assert torch.equal(pad_packed_sequence(mine, batch_first=True)[0], want_pad)
        assert torch.equal(torch.from_numpy(ET.padded(arena, off, lens, max_len))[:, :tmax], want_pad)


def test_pair_fuse_special_table_matches_the_oracle(oracle):
    l1, l2 = special_table()
    assert l1.shape == (11 ** 4, 2)
    seen = set()
    for mode in MODES:
        got = ET.pair_fuse(l1, l2, mode)
        assert got.dtype == np.int8 and (got == oracle.pair_fuse(l1, l2, mode)).all(), mode
        seen |= set(got.tolist())
    assert seen == {0, 1, -1}
    # the rounding case the table is there for: 2^24 + 1 rounds to 2^24, so the sums tie in fp32 where the exact sums do not
    a, b = np.array([[2.0 ** 24, 2.0 ** 24]], dtype=np.float32), np.array([[0.0, 1.0]], dtype=np.float32)
    assert ET.pair_fuse(a, b, "none")[0] == 0 and float(a[0, 1]) + float(b[0, 1]) > float(a[0, 0]) + float(b[0, 0])


@pytest.mark.parametrize("n", [1, 2, 3, 257, 5000])
def test_pair_fuse_and_count_match_the_oracle(oracle, n):
    l1, l2 = tied_logits(n, seed=n)
    for mode in MODES:
        lab = ET.pair_fuse(l1, l2, mode)
        assert (lab == oracle.pair_fuse(l1, l2, mode)).all(), mode
        assert ET.fuse_counts(lab) == oracle.count_labels(lab)                    # int8 labels: the oracle defines 0, 1 and -1
        c0, c1 = ET.count(lab.view(np.uint8))
        assert [c0, c1] == oracle.count_labels(lab)[:2]
    if n == 5000:
        k = [int(((l1[:, 1] == l1[:, 0])).sum()), int((l2[:, 1] == l2[:, 0]).sum()),
             int((l1[:, 0] + l2[:, 0] == l1[:, 1] + l2[:, 1]).sum())]
        assert min(k) > 40 and sum(k) > 0.04 * n, k


def test_count_ignores_other_values():
    lab = np.array([0, 1, 2, 127, 128, 255, 1, 0, 0], dtype=np.uint8)
    assert ET.count(lab) == (3, 2) and ET.count(lab[:0]) == (0, 0)
