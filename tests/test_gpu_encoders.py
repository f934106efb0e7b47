"""The kernels behind the reference's own tensor layouts (include/ribodetector_amd.h: rd_pack_plan, rd_pack_onehot,
rd_encode_onehot_padded, rd_encode_codes) against the plain numpy statements in tests/encoder_truth.py, at the sizes where their
code paths change: more than one block of the stable sort (2,048 reads), more than 256 blocks and more than 256 lengths in its
scans, more than one workgroup (64 reads) and more than one 128-step chunk of the packer, max_len above 256 in the padded encoder,
and the 16,384-workgroup grid cap of both encoders. Everything is exact equality, compared on the device; outputs are poisoned
first and fenced with guard rows. Last, rd_classify's own bucketing by step count (csrc/rd_sort.hpp) past one grid-stride pass on
reads of mixed lengths, where every row of the batch can be checked because it repeats a read of a small pool."""
import os

import numpy as np
import pytest
import torch

import encoder_truth as ET
from test_encoder_truth_host import place_reads, ragged_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RD_E_INVALID, RD_E_WORKSPACE = -1, -4
MAX_LEN_LIMIT = 16000
N_BLOCKS_257 = 256 * 2048 + 1        # 257 blocks of the sort: two counts per lane in the row scan
N_GRID = 16384 * 64 + 65             # past the encoders' grid cap: 16,384 workgroups of 64 reads, then the grid-stride loop
GUARD = 64
SENTINEL = -7


def _native():
    from ribodetector_amd import _native as N
    return N, N.lib()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    """exact equality on the device; only the first differences travel to the host"""
    want = want if torch.is_tensor(want) else _up(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g, w = got.reshape(-1), want.reshape(-1)
    bad = torch.nonzero(g != w)[:, 0]
    at = bad[:6]
    raise AssertionError("%s: %d of %d elements differ, first at %s: got %s, want %s"
                         % (what, bad.numel(), g.numel(), at.cpu().tolist(), g[at].cpu().tolist(), w[at].cpu().tolist()))


def _plan_outputs(n, max_len):
    return [torch.full((k,), SENTINEL, dtype=torch.int64, device=DEV) for k in (n, n, max_len, 1)]


def run_plan(lens_d, n, max_len):
    N, L = _native()
    ws = torch.empty(int(L.rd_classify_workspace_bytes(n, max_len)), dtype=torch.uint8, device=DEV)
    si, ui, bs, tot = _plan_outputs(n, max_len)
    with torch.cuda.device(DEV):
        N.check(L.rd_pack_plan(N.ptr(lens_d), n, max_len, N.ptr(si), N.ptr(ui), N.ptr(bs), N.ptr(tot), N.ptr(ws), ws.numel(),
                               N.stream_ptr(DEV)), "rd_pack_plan")
    return si, ui, bs, tot


def check_plan(lens, max_len, what):
    n = len(lens)
    order, inverse, sizes, total = ET.pack_plan(lens, max_len)
    si, ui, bs, tot = run_plan(_up(lens), n, max_len)
    _same(si, order, "%s: sorted_idx" % (what,))
    _same(ui, inverse, "%s: unsorted_idx" % (what,))
    assert torch.equal(ui[si], torch.arange(n, device=DEV)), what
    _same(bs, sizes, "%s: batch_sizes" % (what,))
    assert int(tot.item()) == total, (what, int(tot.item()), total)
    return si, ui, bs, total


def length_pattern(name, n, max_len, rng):
    i = np.arange(n, dtype=np.int64)
    if name == "equal":
        v = np.full(n, max(1, max_len // 2))
    elif name == "zero":
        v = np.zeros(n)
    elif name == "above":
        v = rng.integers(max_len + 1, 2 ** 31, size=n)
    elif name == "negative":                          # a quarter negative: they clamp to 0
        v = np.where(rng.random(n) < 0.25, rng.integers(-2 ** 31, 0, size=n), rng.integers(0, 2 * max_len + 1, size=n))
    elif name == "ascending":
        v = i
    elif name == "descending":
        v = i[::-1]
    elif name == "alternating":                       # two values in turn: each tie group runs through every block boundary
        v = np.where(i % 2 == 0, max_len // 3, max_len)
    elif name == "random":
        v = rng.integers(0, 2 * max_len + 1, size=n)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(v, dtype=np.int32)


PATTERNS = ["equal", "zero", "above", "negative", "ascending", "descending", "alternating", "random"]


# ---- rd_pack_plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4097, N_BLOCKS_257])
def test_pack_plan_read_counts(n):
    """one block, the block boundary, two and three blocks, 257 blocks (max_len 16)"""
    check_plan(length_pattern("random", n, 16, np.random.default_rng(n)), 16, "n=%d" % n)


@pytest.mark.parametrize("max_len", [1, 2, 8, 254, 255, 256, 257, 300, 1000, MAX_LEN_LIMIT])
def test_pack_plan_max_len(max_len):
    """max_len + 1 lengths: up to 256 (one per lane of the start scan), more than 256, and the limit (a 64,004-byte LDS histogram)"""
    check_plan(length_pattern("random", 4097, max_len, np.random.default_rng(max_len)), max_len, "max_len=%d" % max_len)


@pytest.mark.parametrize("n,max_len", [(4097, 300), (4097, 5000), (N_BLOCKS_257, 16)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pack_plan_length_patterns(pattern, n, max_len):
    """(4097, 5000): ascending and descending lengths are all distinct there; (4097, 300) and 257 blocks: they clamp into ties"""
    lens = length_pattern(pattern, n, max_len, np.random.default_rng(5))
    si, _, _, _ = check_plan(lens, max_len, "%s n=%d max_len=%d" % (pattern, n, max_len))
    if pattern == "alternating":                      # stability said once more without the reference: each half in input order
        assert torch.equal(si[:n // 2], torch.arange(1, n, 2, device=DEV)) and torch.equal(si[n // 2:], torch.arange(0, n, 2, device=DEV))


def test_pack_plan_rejected_arguments():
    N, L = _native()
    n, max_len = 100, 16
    lens = _up(length_pattern("random", n, max_len, np.random.default_rng(0)))
    need = int(L.rd_classify_workspace_bytes(n, max_len))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = _plan_outputs(n, max_len)
    big = _plan_outputs(n, MAX_LEN_LIMIT + 1)
    ws_big = torch.empty(int(L.rd_classify_workspace_bytes(n, MAX_LEN_LIMIT + 1)) + 65536, dtype=torch.uint8, device=DEV)

    def call(lens=lens, n=n, max_len=max_len, outs=outs, ws=ws, ws_bytes=need):
        with torch.cuda.device(DEV):
            rc = L.rd_pack_plan(N.ptr(lens), n, max_len, *[N.ptr(t) for t in outs], N.ptr(ws), ws_bytes, N.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    assert call(max_len=MAX_LEN_LIMIT + 1, outs=big, ws=ws_big, ws_bytes=ws_big.numel()) == RD_E_INVALID
    assert call(max_len=0) == RD_E_INVALID
    assert call(n=0) == RD_E_INVALID
    assert call(lens=None) == RD_E_INVALID
    assert call(ws=None) == RD_E_INVALID
    for k in range(4):
        assert call(outs=[None if j == k else t for j, t in enumerate(outs)]) == RD_E_INVALID, k
    assert call(ws_bytes=need - 1) == RD_E_WORKSPACE
    assert b"workspace" in L.rd_last_error()
    for t in outs + big:                              # no refused call wrote anything
        assert bool((t == SENTINEL).all())
    assert call() == 0                                # and the same arguments with the whole workspace are accepted
    assert int(outs[3].item()) == ET.pack_plan(lens.cpu().numpy(), max_len)[3]


# ---- rd_pack_onehot ------------------------------------------------------------------------------------------------------------
def check_pack(arena, off, lens, max_len, what):
    """the kernel's own plan -> rd_pack_onehot into a NaN-poisoned buffer with GUARD rows on either side"""
    N, L = _native()
    n = len(lens)
    a, o, ln = _up(arena), _up(off), _up(lens)
    si, _, bs, total = check_plan(lens, max_len, what)
    buf = torch.full((total + 2 * GUARD, 4), float("nan"), dtype=torch.float32, device=DEV)
    data = buf[GUARD:GUARD + total]
    if total:
        with torch.cuda.device(DEV):
            N.check(L.rd_pack_onehot(N.ptr(a), N.ptr(o), N.ptr(ln), n, max_len, N.ptr(si), N.ptr(bs), N.ptr(data), N.stream_ptr(DEV)),
                    "rd_pack_onehot")
    assert not bool(torch.isnan(data).any()), "%s: rows left unwritten" % (what,)
    _same(data, ET.pack_data(arena, off, lens, max_len), "%s: data" % (what,))
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + total:]).all()), "%s: wrote outside its rows" % (what,)
    return total


@pytest.mark.parametrize("n", [1, 64, 65, 127, 128, 129, 4097])
def test_pack_onehot_read_counts(n):
    """one workgroup (64 sorted reads), a partly filled second one, exactly two, 65 of them"""
    arena, off, lens = ragged_batch(n, 20, seed=n, lo=1 if n == 1 else 0)
    check_pack(arena, off, lens, 20, "n=%d" % n)


@pytest.mark.parametrize("max_len", [127, 128, 129, 256, 257, 600])
def test_pack_onehot_step_chunks(max_len):
    """up to 128 steps are one chunk; past that the row offset is carried from chunk to chunk"""
    arena, off, lens = ragged_batch(200, max_len, seed=max_len)
    assert lens.max() >= max_len
    check_pack(arena, off, lens, max_len, "max_len=%d" % max_len)


def test_pack_onehot_empty_reads():
    from ribodetector_amd.data_loader import seq_encoder as E
    arena, off, lens = ragged_batch(300, 20, seed=4, lo=1)
    lens[np.random.default_rng(4).permutation(300)[:100]] = 0      # the last 100 sorted reads: the fifth workgroup has only empty ones
    assert check_pack(arena, off, lens, 20, "100 empty reads") > 0
    lens[:] = 0                                                     # all empty: nothing to pack, the packer is not launched
    assert check_pack(arena, off, lens, 20, "all empty") == 0
    p = E.pack_reads(E.ReadBatch(_up(arena), _up(off), _up(lens)), 20)
    assert tuple(p.data.shape) == (0, 4) and p.batch_sizes.numel() == 0
    assert torch.equal(p.sorted_indices, torch.arange(300, device=DEV)) and torch.equal(p.unsorted_indices, torch.arange(300, device=DEV))
    for base in b"GN":                                              # a single read of one base
        one = np.array([base], dtype=np.uint8)
        assert check_pack(one, np.zeros(1, np.int64), np.ones(1, np.int32), 20, "one base") == 1
        p = E.pack_reads(E.batch_from_strings([bytes([base])], DEV), 20)
        assert p.data.cpu().tolist() == [[0.0, 0.0, 1.0 if base == ord("G") else 0.0, 0.0]] and p.batch_sizes.tolist() == [1]


def test_pack_reads_matches_torch_pack_sequence():
    """pad_packed_sequence does not depend on the order of ties, which torch leaves open"""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    from ribodetector_amd.data_loader import seq_encoder as E
    arena, off, lens = ragged_batch(300, 20, seed=9, lo=1)
    for max_len in (20, 45):
        T = ET.steps(lens, max_len)
        want = pack_sequence([torch.from_numpy(ET.ONEHOT[ET.LUT[arena[off[i]:off[i] + T[i]]]]) for i in range(300)], enforce_sorted=False)
        got = E.pack_reads(E.ReadBatch(_up(arena), _up(off), _up(lens)), max_len).to("cpu")
        assert torch.equal(got.batch_sizes, want.batch_sizes)
        g, gl = pad_packed_sequence(got, batch_first=True)
        w, wl = pad_packed_sequence(want, batch_first=True)
        assert torch.equal(g, w) and torch.equal(gl, wl)


# ---- rd_encode_onehot_padded ---------------------------------------------------------------------------------------------------
def check_padded(a, o, lens, max_len, want, what):
    N, L = _native()
    n = len(lens)
    buf = torch.full((n * max_len + 2 * GUARD, 4), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n * max_len]
    with torch.cuda.device(DEV):
        N.check(L.rd_encode_onehot_padded(N.ptr(a), N.ptr(o), N.ptr(_up(lens)), n, max_len, N.ptr(out), N.stream_ptr(DEV)),
                "rd_encode_onehot_padded")
    _same(out.view(n, max_len, 4), want, "%s: one-hot" % (what,))
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n * max_len:]).all()), "%s: wrote outside its rows" % (what,)


@pytest.mark.parametrize("max_len", [1, 2, 3, 7, 64, 100, 255, 256, 257, 300, 1000])
def test_padded_max_len(max_len):
    """max_len up to 256 steps (read, row) by 256 / max_len reads and 256 % max_len rows per pass; above 256 it walks one read"""
    for n in (1, 63, 64, 65, 130):
        arena, off, lens = ragged_batch(n, max_len, seed=1000 * max_len + n)
        check_padded(_up(arena), _up(off), lens, max_len, ET.padded(arena, off, lens, max_len), "max_len=%d n=%d" % (max_len, n))


@pytest.fixture(scope="module")
def grid_batch():
    """N_GRID read slots of 32 bytes over all 256 byte values, read i at 32 i + i mod 16"""
    rng = np.random.default_rng(21)
    arena, off, _ = place_reads(np.full(N_GRID, 16, dtype=np.int32), rng, slot=32)
    return arena, off, _up(arena), _up(off)


def test_padded_past_the_grid_cap(grid_batch):
    arena, off, a, o = grid_batch
    lens = np.random.default_rng(22).integers(0, 6, size=N_GRID).astype(np.int32)
    check_padded(a, o, lens, 3, ET.padded(arena, off, lens, 3), "n=%d max_len=3" % N_GRID)


# ---- rd_encode_codes -----------------------------------------------------------------------------------------------------------
def check_codes(a, o, lens, max_len, stride, want, what):
    N, L = _native()
    n = len(lens)
    buf = torch.full((n * stride + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + n * stride]
    with torch.cuda.device(DEV):
        N.check(L.rd_encode_codes(N.ptr(a), N.ptr(o), N.ptr(_up(lens)), n, max_len, stride, N.ptr(out), N.stream_ptr(DEV)), "rd_encode_codes")
    _same(out.view(n, stride), want, "%s: codes" % (what,))
    assert bool((buf[:GUARD] == 0xEE).all()) and bool((buf[GUARD + n * stride:] == 0xEE).all()), "%s: wrote outside its rows" % (what,)


@pytest.mark.parametrize("stride", [5, 8])
def test_codes_past_the_grid_cap(grid_batch, stride):
    """stride 5: byte stores; stride 8 (a multiple of 4 on an aligned output): dword stores"""
    arena, off, a, o = grid_batch
    lens = np.random.default_rng(23).integers(0, 9, size=N_GRID).astype(np.int32)
    check_codes(a, o, lens, 5, stride, ET.codes(arena, off, lens, 5, stride), "n=%d stride=%d" % (N_GRID, stride))


@pytest.mark.parametrize("max_len,stride", [(16, 16), (16, 17), (16, 20), (17, 17), (17, 20)])
def test_codes_around_one_piece(max_len, stride):
    """reads of 15, 16 and 17 bases, each at every arena offset mod 16: a whole 16-byte piece, the piece that holds the read's end, the
    byte loop of a read under 16 bases"""
    lens = np.tile(np.array([15, 16, 17], dtype=np.int32), 32)
    arena, off, lens = place_reads(lens, np.random.default_rng(24))
    assert {(int(ln), int(of) % 16) for ln, of in zip(lens, off)} == {(ln, k) for ln in (15, 16, 17) for k in range(16)}
    assert set(arena.tolist()) == set(range(256))
    check_codes(_up(arena), _up(off), lens, max_len, stride, ET.codes(arena, off, lens, max_len, stride), "max_len=%d stride=%d" % (max_len, stride))


# ---- the bucketing inside rd_classify ------------------------------------------------------------------------------------------
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
POOL, POOL_ROW, POOL_MAX_LEN = 4096, 40, 24
N_BUCKETS = 256 * 2048 * 2 + 777      # more than two passes of the 256 scatter workgroups of 2,048 reads


@pytest.fixture(scope="module")
def model():
    from ribodetector_amd.model import model as module_arch
    from ribodetector_amd.parse_config import ConfigParser
    cfg = ConfigParser.from_json(os.path.join(ROOT, "ribodetector_amd", "config.json"))
    m = cfg.init_obj("arch", module_arch)
    m.load_state_dict(cfg.load_state_dict("mcc"))
    m.set_prefix_table(0)
    return m.to(DEV).eval()


def pool_reads():
    """4,096 reads of 0...40 bases (different ones wherever the length allows), one per 40-byte row: a tenth with an N among the first 12 bases, some all N, some empty"""
    rng = np.random.default_rng(41)
    rows = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(POOL, POOL_ROW))]
    lens = rng.integers(0, POOL_ROW + 1, size=POOL).astype(np.int32)
    hit = np.flatnonzero(rng.random(POOL) < 0.1)
    rows[hit, rng.integers(0, 12, size=len(hit))] = ord("N")
    for i in range(5, POOL, 97):
        rows[i, :lens[i]] = ord("N")
    lens[3::101] = 0
    return rows, lens


@pytest.fixture(scope="module")
def pool():
    rows, lens = pool_reads()
    reads = {bytes(r[:ln]) for r, ln in zip(rows, lens)}
    assert (lens == 0).sum() > 40 and len(reads) > POOL - 400, len(reads)       # (the empty read and the shortest ones repeat)
    return _up(rows.reshape(-1)), torch.arange(POOL, dtype=torch.int64, device=DEV) * POOL_ROW, _up(lens)


@pytest.mark.parametrize("sem,variant,prefix_k", [("packed", "auto", 0), ("padded", "auto", 0), ("packed", "mfma_f32", 0),
                                                  ("padded", "mfma_f32", 0), ("packed", "auto", 12)])
def test_classify_buckets_every_read_once(model, pool, sem, variant, prefix_k):
    """every row of a 1,049,353-read call equals, bit for bit, the row of the pool read it repeats (batch-split invariance, which
    tests/test_gpu_parity.py asserts at 5,000 reads): a read that the bucketing dropped, duplicated or misplaced shows up. Lengths of
    all 41 values (the per-lane atomics of the bin counter and many bins), then of two values only (few bins, mixed waves)."""
    arena, off, lens = pool
    model.set_variant(variant)
    model.set_semantics(sem)
    try:
        model.set_prefix_table(prefix_k)
        assert model.prefix_k == prefix_k
        lg, lb = model.classify_bytes(arena, off, lens, POOL_MAX_LEN)
        model.sync_results()
        lg, lb = lg.clone(), lb.clone()
        assert torch.equal((lg[:, 1] > lg[:, 0]).to(torch.uint8), lb) and 0 < int(lb.sum()) < POOL
        g = torch.Generator(device=DEV)
        g.manual_seed(43)
        two = torch.nonzero((lens == 17) | (lens == 30))[:, 0]
        assert two.numel() > 100
        for what, draw in (("all lengths", torch.randint(0, POOL, (N_BUCKETS,), device=DEV, generator=g)),
                           ("two lengths", two[torch.randint(0, two.numel(), (N_BUCKETS,), device=DEV, generator=g)])):
            big_lg = torch.full((N_BUCKETS, 2), float("nan"), dtype=torch.float32, device=DEV)
            big_lb = torch.full((N_BUCKETS,), 0xEE, dtype=torch.uint8, device=DEV)
            model.classify_bytes(arena, off[draw].contiguous(), lens[draw].contiguous(), POOL_MAX_LEN, logits=big_lg, labels=big_lb)
            model.sync_results()
            bad = torch.nonzero((big_lg != lg[draw]).any(1) | (big_lb != lb[draw]))[:, 0]
            assert bad.numel() == 0, "%s: %d rows differ from their pool read, first %s (pool reads %s)" % (
                what, bad.numel(), bad[:6].cpu().tolist(), draw[bad[:6]].cpu().tolist())
            assert torch.equal(big_lg, lg[draw]) and torch.equal(big_lb, lb[draw])
    finally:
        model.set_semantics("packed")
        model.set_prefix_table(0)
        model.set_variant("auto")
