"""The decimal -> float32 conversion on the GPU: C ABI rd_float_parse (csrc/rd_float_parse.hpp, one lane per value) against the rule
bam.float_from_text, bit for bit, through ubam.float_parse and through the library itself.

Launch shape: 256 threads per workgroup, at most 1,024 workgroups that stride over the values - 2^16 texts are 256 workgroups, five
copies of them one more trip of the stride for a quarter of the lanes."""
import numpy as np
import pytest

import bam_float_cases as F
import float_parse_cases as C
from ribodetector_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5


def _want(rule):
    bits = np.array([0 if r is None or r == C.SKIPPED else r for r in rule], np.uint32)
    status = np.array([1 if r is None else 2 if r == C.SKIPPED else 0 for r in rule], np.uint8)
    return bits, status


def _compare(texts, rule):
    import torch
    from ribodetector_amd import ubam
    with torch.cuda.device(DEV):
        bits, status = ubam.float_parse(texts)
    wb, ws = _want(rule)
    bad = np.flatnonzero((bits != wb) | (status != ws))
    assert not len(bad), "%d of %d differ, first %r: got 0x%08x status %d, want 0x%08x status %d" % (
        len(bad), len(texts), texts[bad[0]], bits[bad[0]], status[bad[0]], wb[bad[0]], ws[bad[0]])


def test_the_hard_and_the_syntax_tables():
    texts = [t for t, _ in C.HARD]
    _compare(texts, [w for _, w in C.HARD])                # the table's own results, by hand
    texts = [t for t, _ in C.SYNTAX] + [b"-" + t for t, _ in C.SYNTAX]
    rule = C.rule("syntax", texts)
    assert [r is not None for r in rule[:len(C.SYNTAX)]] == [ok for _, ok in C.SYNTAX]
    _compare(texts, rule)


def _generated():
    mids = C.midpoint_texts(4, 6) + C.exact_midpoints()[::4]
    texts = [t for t, _ in mids]
    for fmt in ("%g", "%.9g", "%.17g"):
        texts += C.pattern_texts(F.sweep(2, 4) + F.randoms(7, 1 << 12), fmt)[0]
    texts += [t for _, _, _, t in C.random_texts(19, (1 << 16) - len(texts))]
    assert len(texts) == 1 << 16
    return texts, [w for _, w in mids]


def test_65536_generated_texts_and_a_second_trip_of_the_stride():
    texts, mids = _generated()
    rule = C.rule("gpu generated", texts)
    assert rule[:len(mids)] == mids
    _compare(texts, rule)
    starts = np.cumsum([0] + [len(t) for t in texts[:-1]])
    assert set((starts % 16).tolist()) == set(range(16)), "values start on every residue modulo 16"
    _compare(texts * 5, rule * 5)


def _call(text, start, n, guard=64):
    """the library itself on a text buffer that ends with its last value; returns (bits, status) and the bytes behind both"""
    import torch
    t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(DEV)
    s = torch.from_numpy(np.asarray(start, np.int64)).to(DEV)
    bits = torch.full((n + guard,), -1515870811, dtype=torch.int32, device=DEV)       # 0xA5A5A5A5
    status = torch.full((n + guard,), CANARY, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        N.check(N.lib().rd_float_parse(N.ptr(t), N.ptr(s), n, N.ptr(bits), N.ptr(status), N.stream_ptr(torch.device(DEV))), "rd_float_parse")
    torch.cuda.synchronize()
    b, st = bits.cpu().numpy().view(np.uint32), status.cpu().numpy()
    assert (b[n:] == 0xA5A5A5A5).all() and (st[n:] == CANARY).all(), "written behind the n values"
    return b[:n], st[:n]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_value_counts_around_a_wave(n):
    texts = [t for _, _, _, t in C.random_texts(23, n)]
    rule = C.rule("wave %d" % n, texts)
    start = np.cumsum([0] + [len(t) for t in texts])
    bits, status = _call(b"".join(texts), start, n)
    wb, ws = _want(rule)
    assert np.array_equal(bits, wb) and np.array_equal(status, ws)


def test_every_start_residue_with_the_value_at_the_buffers_end():
    """a value of every length 1..24 behind a filler of every length 0..15: the last value ends with the buffer"""
    pool = [b"7"] + [t for _, _, _, t in C.random_texts(29, 4000)] + [t for t, _ in C.HARD]
    by_len = {}
    for t in pool:
        by_len.setdefault(len(t), t)
    for pad in range(16):
        texts = [b"1" * pad] + [by_len[k] for k in range(1, 25)]
        for last in (by_len[1], by_len[16], by_len[24], b"1e", b"5.", b"1e+", b"-", b"in", b"1.0000000596046448"):
            seq = texts + [last]
            start = np.cumsum([0] + [len(t) for t in seq])
            bits, status = _call(b"".join(seq), start, len(seq))
            wb, ws = _want(C.rule("residue %d %r" % (pad, last), seq))
            assert np.array_equal(bits, wb) and np.array_equal(status, ws), (pad, last)


def test_the_table_is_held_against_its_last_entry():
    text = b"1.5,2.5,3.5"
    start = [0, 3, 4, 7, 8, 11]
    bits, status = _call(text, start, 5)
    assert status.tolist() == [0, 1, 0, 1, 0] and bits.tolist() == [0x3fc00000, 0, 0x40200000, 0, 0x40600000]
    # entries that run backwards, are negative or lie behind the last one: status 1, nothing read
    bits, status = _call(text, [0, 3, 2, 1 << 40, -5, 11], 5)
    assert status.tolist() == [0, 1, 1, 1, 1] and bits.tolist() == [0x3fc00000, 0, 0, 0, 0]


def test_no_values_and_null_pointers():
    import torch
    L = N.lib()
    assert L.rd_float_parse(None, None, 0, None, None, None) == 0                 # n == 0: a no-op
    t = torch.zeros(16, dtype=torch.uint8, device=DEV)
    s = torch.zeros(2, dtype=torch.int64, device=DEV)
    b = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = [N.ptr(t), N.ptr(s), 1, N.ptr(b), N.ptr(t), None]
    for k in (0, 1, 3, 4):
        bad = list(args)
        bad[k] = None
        assert L.rd_float_parse(*bad) == -1 and b"rd_float_parse" in L.rd_last_error()
    assert L.rd_float_parse(N.ptr(t), N.ptr(s), -1, N.ptr(b), N.ptr(t), None) == -1
    from ribodetector_amd import ubam
    with torch.cuda.device(DEV):
        bits, status = ubam.float_parse([])
    assert len(bits) == 0 and len(status) == 0
