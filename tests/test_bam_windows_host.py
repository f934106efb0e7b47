"""The inputs of tests/test_gpu_bam_index.py are what those tests assume - proven here with the rule (bam.records) alone, no GPU: records
start at the intended offsets and not at the decoys, windows have the intended number of segments, spanning records cover the intended
segments, the dense windows overflow the reader's first record table - and check(), the comparator of the GPU tests, rejects every
single-entry perturbation of expect()'s output (no deliberately broken kernel runs anywhere)."""
import copy
import struct

import numpy as np
import pytest

import bam_windows as W
from ribodetector_amd import bam

S = W.S


def _hold(w, want, nseg=None):
    """the window is what its builder intends: record starts at the targets, none at the decoys (whose own chain meets the true one
    exactly when `rejoin`), the spanning records where they belong"""
    starts = set(want["offsets"]) | {want["consumed"]}
    assert all(t in starts for t in w.targets), [t for t in w.targets if t not in starts]
    if nseg is not None:
        assert w.nseg == nseg, (w.nseg, nseg)
    for off, rejoin in w.decoys:
        assert off % S == 0 and off not in starts
        chain = []
        try:
            for r in bam.records(w.data, start=off):
                chain.append(r.offset)
                if len(chain) == 4:
                    break
        except ValueError:
            pass
        assert chain[:1] == [off]
        assert (len(chain) == 4 and all(o in starts for o in chain[1:])) if rejoin else len(chain) == 1
    for start, size in w.spans:
        assert start in starts and start + size in starts


def test_builders():
    rng = np.random.default_rng(1)
    for size, name in ((42, b"f"), (48, b"f"), (3000, b"f123"), (5 * (1 << 20) + 3, b"span")):
        rec = W.filler(size, name)
        got = list(bam.records(rec, start=0))
        assert len(rec) == size and len(got) == 1 and got[0].name == name and got[0].size == size and got[0].fastq() == b"@" + name + b"\n\n+\n\n"
    for named, size, text in ((False, 37, 6), (True, 38, 7)):
        recs = W.tiny(5, named)
        assert all(len(r) == size for r in recs) and all(len(r.fastq()) == text for r in bam.records(b"".join(recs), start=0))
    read = W.G._read_of(rng, 30, name=b"abc", kind=1)
    u = W.unprintable(read, rng)
    assert len(u["name"]) == 3 and all(not 33 <= c <= 126 and c != 0 for c in u["name"]) and u["seq"] == read["seq"]
    assert len(W.unprintable(dict(read, name=b""), rng)["name"]) == 1
    far = W.far_fields(read)
    assert [struct.unpack_from("<i", far, at)[0] for at in (4, 8, 24, 28)] == [-2] * 4
    assert [r.fastq() for r in bam.records(far, start=0)] == [r.fastq() for r in bam.records(bam.encode_record(read), start=0)]
    assert len(W.long_name()) == W.LONG_SIZE and W.long_name()[12] == 255
    targets = [5000, 5048, 3 * S - 4, 3 * S + 44, 5 * S]
    recs = W.place(targets, seed=2)
    offs = [r.offset for r in bam.records(b"".join(recs) + W.filler(48), start=0)]
    assert all(t in offs for t in targets) and sum(len(r) for r in recs) == 5 * S
    for rejoin in (False, True):
        start, host, decoy = W.decoy_at(7 * S, rejoin)
        assert start == 7 * S - W.LEAD and [r.name for r in bam.records(host, start=0)] == [b"host"]
        assert [r.name for r in bam.records(host if rejoin else decoy, start=W.LEAD if rejoin else 0)] == [b"decoy"]


@pytest.mark.parametrize("k", range(len(W.ROUND_EDGES)))
def test_round_edge_windows(k):
    length = W.ROUND_EDGES[k]
    w = W.round_edge(length)
    want = W.expect(w.data, 1)
    assert len(w.data) == length == want["consumed"] and want["status"] == 0
    _hold(w, want, nseg=[64, 64, 65, 128, 128, 129, 65, 129][k])
    assert (64 * S in w.targets) == (k in (1, 3, 4, 5, 6, 7)) and (128 * S in w.targets) == (k in (4, 7))
    assert want["n_lines"] > want["n_records"] > 1000                       # (reads of the skipped kinds among them)


def test_decoy_windows():
    for j in W.DECOY_J:
        for rejoin in (False, True):
            w = W.decoys((j,), (rejoin,))
            want = W.expect(w.data, 1)
            assert want["status"] == 0 and w.decoys == [(j * S, rejoin)]
            _hold(w, want, nseg=130)
    for j1, r1, j2, r2 in W.TWO_DECOYS:
        w = W.decoys((j1, j2), (r1, r2))
        assert w.decoys == [(j1 * S, r1), (j2 * S, r2)]
        _hold(w, W.expect(w.data, 1), nseg=130)
    # the rounds of 64 segments the decoys fall into: one alone in round 0 (1, 63), in round 1 (64, 65, 127), in round 2 (128); two
    # in rounds 0 and 1 - between them: serial then fast, fast then serial, serial then serial
    assert sorted({j // 64 for j in W.DECOY_J}) == [0, 1, 2] and [(a // 64, b // 64) for a, _, b, _ in W.TWO_DECOYS] == [(0, 1), (0, 1)]


def test_spanning_windows():
    segs = {"62_to_66": (62, 66), "60_to_130": (60, 130), "0_for_70": (0, 70)}
    for tag, (start, size, n) in W.SPANS.items():
        w = W.spanning(tag)
        want = W.expect(w.data, 1)
        _hold(w, want, nseg=n)
        assert w.spans == [(start, size)] and (start // S, (start + size - 1) // S) == segs[tag]
        k = want["offsets"].index(start)
        assert k >= 3 and len(want["offsets"]) - k > 3 and want["n_records"] > 3       # (reads in front of it and behind it)


def test_guess_proof_windows():
    w = W.guess_proof("unprintable")
    recs = list(bam.records(w.data, start=0))
    assert w.nseg == 70 and all(len(r.name) >= 1 and all(c in W.UNPRINTABLE for c in r.name) for r in recs)
    w = W.guess_proof("far")
    recs = list(bam.records(w.data, start=0))
    assert w.nseg == 70 and all(struct.unpack_from("<ii", w.data, r.offset + 4) == struct.unpack_from("<ii", w.data, r.offset + 24) == (-2, -2) for r in recs)
    assert len({r.offset // S for r in recs}) == 70


def test_dense_windows_overflow_the_first_tables():
    for behind, nseg in ((False, 46), (True, 110)):
        w = W.dense(behind)
        want = W.expect(w.data, 1)
        assert w.nseg == nseg and want["n_records"] >= 40000 and (behind or len(want["norm"]) % 16 == 0)
        _hold(w, want)
    full = [o // S for o in W.expect(W.dense(False).data, 1)["offsets"]]
    assert max(np.bincount(full)) == S // 37 + 1                              # a segment's list filled to its last entry
    for named in (False, True):                                               # the reader-level files of tests/test_gpu_bam.py
        window = sum(len(r) for r in W.tiny(20000, named))
        assert 20000 + 1 > window // 96 + 4096
    assert 40000 + 1 > len(W.dense(False).data) // 96 + 4096


def test_reach_windows():
    for h in (S, 64 * S):
        for d in W.REACH_D:
            for how in ("mid", "last", "cut"):
                w = W.reach(h, d, how)
                want = W.expect(w.data, 1)
                if how == "cut":
                    assert want["consumed"] == h - d and len(w.data) == h - d + 136 and want["status"] == W.N.BAM_TRUNCATED
                    assert W.expect(w.data, 0)["status"] == 0
                else:
                    assert h - d in want["offsets"] and want["status"] == 0 and bytes(w.data[h - d + 36:h - d + 290]) == W.LONG_NAME
                    assert (want["offsets"][-1] == h - d) == (how == "last")


def test_ends_damage_and_ordinary_windows():
    w, at, size = W.ends_chain()
    want = W.expect(w.data, 1)
    assert w.nseg == 66 and at in want["offsets"] and at // S == 65 and (at + size - 1) // S == 65 and size > 40
    for what in W.G.FAULTS:
        for decoy in (False, True) if what == "no_nul" else (False,):
            w = W.damaged(what, decoy)
            want = W.expect(w.data, 1)
            _hold(w, want, nseg=66)
            assert want["status"] == (W.N.BAM_TRUNCATED if what.startswith("cut") or what == "block=0x7fffffff" else W.N.BAM_RECORD)
            assert want["consumed"] > 65 * S and want["n_lines"] > want["n_records"] > 1000
            assert want["bad_record"] == (-1 if want["status"] == W.N.BAM_TRUNCATED else want["n_lines"])
            assert not decoy or (w.decoys == [(64 * S, False)] and want["consumed"] // S == 65)
    w = W.ordinary()
    assert w.nseg == 66 and len(W.expect(w.data, 1)["norm"]) % 16 == 5


def test_sweep_windows():
    seen = set()
    for seed in range(30):
        w, final = W.sweep(seed)
        want = W.expect(w.data, final)
        assert 66 <= w.nseg <= 70, (seed, w.nseg)
        _hold(w, want)
        seen.add((want["status"], final))
    assert {s for s, _ in seen} == {0, W.N.BAM_RECORD, W.N.BAM_TRUNCATED} and {f for _, f in seen} == {0, 1}


def test_the_comparator_rejects_single_entry_perturbations():
    w = W.ordinary()
    want = W.expect(w.data, 1)
    W.check(copy.deepcopy(want), want)
    n = want["n_records"]
    k = next(i for i in range(n // 2, n - 1) if want["hdr_tab"][i] != want["hdr_tab"][i + 1])

    def perturbed():
        for key in W.FIELDS:
            for d in (-1, 1):
                g = copy.deepcopy(want)
                g[key] += d
                yield "%s%+d" % (key, d), g
        for at in (0, n // 2, n):
            for d in (-1, 1):
                g = copy.deepcopy(want)
                g["rec_tab"][at] += d
                yield "rec_tab[%d]%+d" % (at, d), g
        g = copy.deepcopy(want)
        g["hdr_tab"][[k, k + 1]] = g["hdr_tab"][[k + 1, k]]
        yield "hdr_tab swapped", g
        for at in (0, len(want["norm"]) // 2, len(want["norm"]) - 1):
            g = copy.deepcopy(want)
            b = bytearray(g["norm"])
            b[at] ^= 1
            g["norm"] = bytes(b)
            yield "norm[%d]" % at, g
        g = copy.deepcopy(want)
        g["norm"] = g["norm"][:-1]
        yield "norm short", g
        g = copy.deepcopy(want)
        g["rec_tab"] = g["rec_tab"][:-1]
        yield "rec_tab short", g
    tried = 0
    for what, g in perturbed():
        with pytest.raises(AssertionError):
            W.check(g, want, what)
        tried += 1
    assert tried == 2 * len(W.FIELDS) + 6 + 1 + 3 + 2
