"""The label kernels (include/ribodetector_amd.h: rd_pair_fuse, rd_count_labels) against tests/encoder_truth.py - and through it the
CPU oracle, tests/test_encoder_truth_host.py - on both instantiations of each: the vector one (16-byte aligned inputs) with its odd
tails and the plain one that misaligned pointers select, past one grid-stride pass, on logits that tie, are NaN, signed zeros,
denormal or infinite, on sums that tie only after fp32 rounding, and on label bytes other than 0 and 1. Called through the C ABI,
so that the test owns every pointer. Everything is exact equality."""
import numpy as np
import pytest
import torch

import encoder_truth as ET
from test_encoder_truth_host import MODES, special_table, tied_logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FUSE_N = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 2 ** 17 + 3, 1024 * 2048 * 2 + 5]      # the last: two passes of 1,024 workgroups
COUNT_N = [1, 15, 16, 17, 16383, 16384, 16385, 2 ** 20 + 7, 1024 * 16384 * 2 + 17]
ALIGNMENTS = ["aligned", "logits1[1:]", "logits2[1:]", "odd output"]


def _native():
    from ribodetector_amd import _native as N
    return N, N.lib()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fuse(l1, l2, n, mode, out, counts):
    N, L = _native()
    with torch.cuda.device(DEV):
        N.check(L.rd_pair_fuse(N.ptr(l1), N.ptr(l2), n, N.ENSURE_MODES[mode], N.ptr(out), N.ptr(counts), N.stream_ptr(DEV)), "rd_pair_fuse")


def check_fuse(l1, l2, alignments, what):
    """l1, l2: float32 [n, 2] on the host. Every alignment x every mode: labels, the counters after two calls, a call without
    counters, the guard bytes on either side of the labels"""
    n = len(l1)
    want = {m: ET.pair_fuse(l1, l2, m) for m in MODES}
    want_d = {m: _up(want[m]) for m in MODES}
    # row 0 of each buffer is a spare: [1:] of it starts 8 bytes past a 16-byte boundary
    b1 = torch.cat([torch.zeros((2, 2), device=DEV), _up(l1)])
    b2 = torch.cat([torch.zeros((2, 2), device=DEV), _up(l2)])
    s1 = torch.cat([torch.zeros((1, 2), device=DEV), _up(l1)])
    s2 = torch.cat([torch.zeros((1, 2), device=DEV), _up(l2)])
    for al in alignments:
        a1 = s1[1:] if al == "logits1[1:]" else b1[2:]
        a2 = s2[1:] if al == "logits2[1:]" else b2[2:]
        lead = GUARD + 1 if al == "odd output" else GUARD
        assert a1.data_ptr() % 16 == (8 if al == "logits1[1:]" else 0) and a2.data_ptr() % 16 == (8 if al == "logits2[1:]" else 0)
        for mode in MODES:
            buf = torch.full((lead + n + GUARD,), 0x55, dtype=torch.int8, device=DEV)
            out = buf[lead:lead + n]
            assert out.data_ptr() % 2 == (1 if al == "odd output" else 0)
            counts = torch.tensor([3, 5, 7], dtype=torch.int64, device=DEV)
            _fuse(a1, a2, n, mode, out, counts)
            first = out.clone()
            _fuse(a1, a2, n, mode, out, counts)
            tag = "%s, %s, %s" % (what, al, mode)
            if not torch.equal(first, want_d[mode]):
                bad = torch.nonzero(first != want_d[mode])[:6, 0].cpu().numpy()
                raise AssertionError("%s: %d labels differ, first at %s: logits %s %s got %s want %s"
                                     % (tag, int((first != want_d[mode]).sum()), bad.tolist(), l1[bad].tolist(), l2[bad].tolist(),
                                        first.cpu().numpy()[bad].tolist(), want[mode][bad].tolist()))
            assert torch.equal(out, first), tag
            c = ET.fuse_counts(want[mode])
            assert counts.cpu().tolist() == [3 + 2 * c[0], 5 + 2 * c[1], 7 + 2 * c[2]], tag
            assert bool((buf[:lead] == 0x55).all()) and bool((buf[lead + n:] == 0x55).all()), tag + ": wrote outside the labels"
            buf.fill_(0x55)
            _fuse(a1, a2, n, mode, out, None)                      # counts may be null
            assert torch.equal(out, want_d[mode]), tag
            assert bool((buf[:lead] == 0x55).all()) and bool((buf[lead + n:] == 0x55).all()), tag + ": wrote outside the labels"


def test_pair_fuse_special_table():
    """11^4 pairs: every combination of -inf, -1, -0, 0, a denormal, 1, 1 + 2^-23, 2^24, 2^24 + 2, inf and NaN in the four logits
    (odd count: the vector kernel's tail runs too)"""
    l1, l2 = special_table()
    assert len(l1) % 2 == 1
    check_fuse(l1, l2, ALIGNMENTS, "special table")


@pytest.mark.parametrize("n", FUSE_N)
def test_pair_fuse_shapes(n):
    l1, l2 = tied_logits(n, seed=n)
    check_fuse(l1, l2, ALIGNMENTS, "n=%d" % n)


@pytest.fixture(scope="module")
def label_bytes():
    """the largest count's labels plus 15 spare bytes, drawn from {0, 1, 2, 127, 128, 255}"""
    rng = np.random.default_rng(31)
    host = np.array([0, 1, 2, 127, 128, 255], dtype=np.uint8)[rng.integers(0, 6, size=COUNT_N[-1] + 15, dtype=np.uint8)]
    return host, _up(host)


@pytest.fixture(scope="module")
def flat_labels():
    """all 0 and all 1: there every label that a kernel skips or counts twice changes a counter"""
    return torch.zeros(COUNT_N[-1] + 15, dtype=torch.uint8, device=DEV), torch.ones(COUNT_N[-1] + 15, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("n", COUNT_N)
def test_count_labels(label_bytes, flat_labels, n):
    """base 0 is the vector kernel (16 labels per lane, then the n % 16 tail); every other base selects the plain one"""
    N, L = _native()
    host, dev = label_bytes
    assert dev.data_ptr() % 16 == 0 and flat_labels[0].data_ptr() % 16 == 0 and flat_labels[1].data_ptr() % 16 == 0
    for base in range(16):
        c0, c1 = ET.count(host[base:base + n])
        counts = torch.tensor([11, 13, 17], dtype=torch.int64, device=DEV)
        flat = torch.zeros(3, dtype=torch.int64, device=DEV)
        with torch.cuda.device(DEV):
            for _ in range(2):                                 # the counters accumulate
                N.check(L.rd_count_labels(N.ptr(dev[base:base + n]), n, N.ptr(counts), N.stream_ptr(DEV)), "rd_count_labels")
            for t in flat_labels:
                N.check(L.rd_count_labels(N.ptr(t[base:base + n]), n, N.ptr(flat), N.stream_ptr(DEV)), "rd_count_labels")
        assert counts.cpu().tolist() == [11 + 2 * c0, 13 + 2 * c1, 17], (n, base)
        assert flat.cpu().tolist() == [n, n, 0], (n, base)
    if n >= 15:
        assert 0 < c0 < n and 0 < c1 < n and c0 + c1 < n
