"""rd_bam_index below the reader: one call of the C ABI on a window of raw record bytes (tests/bam_windows.py), every output - tables,
text and summary words - against expect(), the rule's serial walk. The windows reach what the reader-level tests of test_gpu_bam.py do
not: stitch rounds behind the first (64 segments of S = bam.SEGMENT bytes per round) with the hand-off between them, the fast path and
the serial loop in either order, records across round boundaries, record starts no guess can find, segment lists filled to their last
entry, a name whose NUL lies at the far end of the staged bytes, every way a window ends, damage behind round one, and tables that are
exactly large enough or one entry short. tests/test_bam_windows_host.py proves the windows are what is assumed here.

Every call: the window at pad = 64 of a zeroed buffer (a chained call: behind a pad sized as the reader's), guards filled with a canary
behind cap_records entries / norm_cap bytes, the call made TWICE into the same buffers - the same bytes both times."""
import numpy as np
import pytest

import bam_windows as W
from ribodetector_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = W.S
LINES = 5                         # RD_FQ_LINES
GUARD, NORM_GUARD = 64, 256
CANARY8, CANARY32, CANARY64 = 0xA5, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _frame(window, final, cap_records=None, norm_cap=None, prev=None):
    """rd_bam_index on `window` (bytes); prev: the `chain` of the call this one chains to. Returns the summary words (consumed counted
    from the window's begin), norm[:reserved], rec_tab[:n + 1], hdr_tab[:n]; asserts the guards and that a second call changes nothing"""
    import torch
    from ribodetector_amd.data_loader.device_reader import PAD
    lib, dev = N.lib(), torch.device(DEV)
    st = N.stream_ptr(dev)
    pad = PAD if prev is not None else 64
    end = pad + len(window)
    text = torch.zeros(((end + 64 + 127) // 64) * 64, dtype=torch.uint8, device=dev)
    if len(window):
        text[pad:end] = torch.from_numpy(np.frombuffer(window, np.uint8).copy()).to(dev)
    size = len(window) + (pad if prev is not None else 0)          # (as FastqIndexer.index: the carry may fill the pad)
    cap_rec = size // 37 + 2 if cap_records is None else cap_records
    ncap = ((4 * size // 3 + 64 + 255) // 256) * 256 if norm_cap is None else norm_cap
    norm = torch.full((ncap + NORM_GUARD,), CANARY8, dtype=torch.uint8, device=dev)
    rec_tab = torch.full((cap_rec + GUARD,), CANARY64, dtype=torch.int64, device=dev)
    hdr_tab = torch.full((cap_rec + GUARD,), CANARY32, dtype=torch.int32, device=dev)
    summary = torch.zeros(8, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.rd_bam_index_workspace_bytes(end)), 256), dtype=torch.uint8, device=dev)
    snaps = []
    for _ in range(2):
        N.check(lib.rd_bam_index(N.ptr(text), pad, end, N.ptr(prev[0]) if prev else None, N.ptr(prev[1]) if prev else None, final, N.ptr(norm), ncap,
                                 N.ptr(rec_tab), N.ptr(hdr_tab), cap_rec, N.ptr(summary), N.ptr(ws), ws.numel(), st), "rd_bam_index")
        torch.cuda.synchronize()
        snaps.append([t.cpu().numpy().copy() for t in (summary, rec_tab, hdr_tab, norm)])
    for a, b, what in zip(snaps[0], snaps[1], ("summary", "rec_tab", "hdr_tab", "norm")):
        assert np.array_equal(a, b), "a second call into the same buffers changed %s" % what
    h, rt, ht, nm = snaps[0]
    assert (nm[ncap:] == CANARY8).all(), "bytes written behind norm_cap"
    assert (rt[cap_rec:] == CANARY64).all() and (ht[cap_rec:] == CANARY32).all(), "entries written behind cap_records"
    begin, wend, n_lines, n, consumed, bad, sd, reserved = (int(x) for x in h)          # (as FastaIndexer._read)
    assert wend == end and 0 <= begin <= pad and 0 <= n < cap_rec and 0 <= reserved <= ncap, (begin, wend, n, reserved)
    return dict(status=sd & 0xffffffff, dirty=(sd >> 32) & 0xffffffff, n_records=n, n_lines=n_lines, consumed=consumed - begin, bad_record=bad, reserved=reserved,
                carry=pad - begin, norm=nm[:reserved].tobytes(), rec_tab=rt[:n + 1], hdr_tab=ht[:n], chain=(text, summary))


def _case(window, final, tag="", dirty=0, **caps):
    got, want = _frame(window, final, **caps), W.expect(window, final)
    W.check(got, want, tag)
    assert int(got["rec_tab"][-1]) == got["reserved"] == len(want["norm"]), tag
    assert got["dirty"] >= dirty, (tag, got["dirty"], dirty)
    return got, want


# ---- rounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", W.ROUND_EDGES, ids=["64S-1", "64S", "64S+1", "128S-1", "128S", "128S+1", "65seg", "129seg"])
def test_round_edges(length):
    for final in (0, 1):
        _case(W.round_edge(length).data, final)


@pytest.mark.parametrize("rejoin", [False, True])
@pytest.mark.parametrize("j", W.DECOY_J)
def test_a_decoy_at_every_round_position(j, rejoin):
    """alone in 130 segments: the round it falls into takes the serial loop, the others the fast path (j < 64: serial then fast;
    64 <= j < 128: fast then serial; 128: fast, fast, serial)"""
    _case(W.decoys((j,), (rejoin,)).data, 1, dirty=1)


@pytest.mark.parametrize("js", W.TWO_DECOYS, ids=["63_65", "1_127"])
def test_two_decoys_serial_then_serial(js):
    j1, r1, j2, r2 = js
    _case(W.decoys((j1, j2), (r1, r2)).data, 1, dirty=2)


@pytest.mark.parametrize("tag", list(W.SPANS))
def test_records_across_rounds(tag):
    for final in (0, 1):
        _case(W.spanning(tag).data, final)


@pytest.mark.parametrize("how", ["unprintable", "far"])
def test_starts_no_guess_finds(how):
    """every record start is rejected by bam_plausible (the walk and the rule accept it): every segment after the first that holds a
    record start is walked again from global memory"""
    w = W.guess_proof(how)
    want = W.expect(w.data, 1)
    _case(w.data, 1, dirty=len({o // S for o in want["offsets"]} - {0}))


@pytest.mark.parametrize("behind", [False, True], ids=["from_0", "behind_64_segments"])
def test_dense_lists(behind):
    _case(W.dense(behind).data, 1)


@pytest.mark.parametrize("d", W.REACH_D)
@pytest.mark.parametrize("h", [S, 64 * S], ids=["S", "64S"])
def test_a_255_byte_name_at_the_end_of_a_segment(h, d):
    for how in ("mid", "last"):
        _case(W.reach(h, d, how).data, 1, tag=how)
    for final in (0, 1):
        _case(W.reach(h, d, "cut").data, final, tag="cut final %d" % final)


# ---- ends -----------------------------------------------------------------------------------------------------------------------------
def test_ends_of_a_66_segment_window():
    w, at, size = W.ends_chain()
    for cut in (at + size // 2, at + 2, at):          # inside a record of segment 65, inside its block_size, exactly on its start
        for final in (0, 1):
            got, want = _case(w.data[:cut], final, tag="cut %d final %d" % (cut - at, final))
            assert want["consumed"] == at and want["status"] == (N.BAM_TRUNCATED if final and cut > at else 0)


def test_a_chained_pair_of_calls_equals_one_call():
    w, at, size = W.ends_chain()
    data, cut = w.data, at + size // 2
    whole = W.expect(data, 1)
    g1, w1 = _case(data[:cut], 0)
    assert w1["consumed"] == at
    rest = data[cut:]
    g2 = _frame(rest, 1, prev=g1["chain"])
    assert g2["carry"] == cut - at
    W.check(g2, W.expect(data[at:], 1), "second call")
    assert g1["norm"] + g2["norm"] == whole["norm"] and g1["n_records"] + g2["n_records"] == whole["n_records"]
    assert g1["n_lines"] + g2["n_lines"] == whole["n_lines"] and g1["consumed"] + g2["consumed"] == whole["consumed"] == len(data)
    assert g2["status"] == whole["status"] == 0
    assert np.array_equal(np.concatenate([g1["rec_tab"][:-1], g2["rec_tab"] + len(g1["norm"])]), whole["rec_tab"])
    assert np.array_equal(np.concatenate([g1["hdr_tab"], g2["hdr_tab"]]), whole["hdr_tab"])


# ---- damage and caps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", W.G.FAULTS)
def test_damage_behind_round_one(what):
    got, want = _case(W.damaged(what).data, 1)
    assert want["n_records"] < want["n_lines"] and want["status"] != 0


def test_damage_in_the_segment_behind_a_decoy():
    _case(W.damaged("no_nul", decoy=True).data, 1, dirty=1)


@pytest.mark.parametrize("which", ["dense", "ordinary"])
def test_tables_exactly_large_enough_and_one_short(which):
    """dense: the text is a multiple of 16 bytes; ordinary: it is not - norm_cap = its length takes the byte tail of the emit pass"""
    w = W.dense(False) if which == "dense" else W.ordinary()
    want = W.expect(w.data, 1)
    n, T = want["n_records"], len(want["norm"])
    assert (T % 16 == 0) == (which == "dense")
    for caps in (dict(cap_records=n + 1), dict(norm_cap=T), dict(cap_records=n + 1, norm_cap=T)):
        _case(w.data, 1, tag=str(caps), **caps)
    for caps in (dict(cap_records=n), dict(norm_cap=T - 1)):
        got = _frame(w.data, 1, **caps)
        assert (got["status"], got["n_records"], got["consumed"], got["reserved"]) == (LINES, 0, 0, 0), (caps, got["status"], got["n_records"], got["consumed"])


# ---- sweep ----------------------------------------------------------------------------------------------------------------------------
def test_seeded_sweep():
    """30 windows (RD_TEST_FULL=1: 300) of 66-70 segments that mix all of the above"""
    from conftest import FULL
    for seed in range(300 if FULL else 30):
        w, final = W.sweep(seed)
        try:
            _case(w.data, final, tag="sweep seed %d" % seed, dirty=len([d for d in w.decoys if d[0] < len(w.data)]))
        except AssertionError:
            print("test_seeded_sweep: failing seed %d (bam_windows.sweep(%d), final %d)" % (seed, seed, final))
            raise
