"""Float BAM tags as %g text on the GPU: the formatter alone (C ABI rd_float_text, csrc/rd_float_text.hpp) and inside the tag splice
(rd_bam_tag_splice_ex with RD_BAM_TAGS_FLOATS; bamtags.splice(floats=True); the CLI's --bam_tag_floats), against the rule in bam.py
(float_g; tag_comment / fastq_text_tagged / tag_counts with floats=True)."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_float_cases as F  # noqa: E402
import bam_tagtext_cases as TC  # noqa: E402
import bam_tags_cases as T  # noqa: E402
from ribodetector_amd import bam  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LANES = [None, "4", "16"]


@pytest.fixture
def lanes(monkeypatch):
    def use(v):
        if v is None:
            monkeypatch.delenv("RD_TAG_LANES", raising=False)
        else:
            monkeypatch.setenv("RD_TAG_LANES", v)
    return use


# ---- the formatter alone ----------------------------------------------------------------------------------------------------------------
def _float_text(patterns, canary=0xa5):
    """rd_float_text over the patterns: (text uint8[n][16], len uint8[n]) as numpy, and the bytes behind both buffers, which hold `canary`"""
    import torch
    from ribodetector_amd import _native as N
    n = len(patterns)
    bits = torch.from_numpy(np.asarray(patterns, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    text = torch.full((16 * n + 64,), canary, dtype=torch.uint8, device=DEV)
    length = torch.full((n + 64,), canary, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        N.check(N.lib().rd_float_text(N.ptr(bits), n, N.ptr(text), N.ptr(length), N.stream_ptr(torch.device(DEV))), "rd_float_text")
    torch.cuda.synchronize()
    text, length = text.cpu().numpy(), length.cpu().numpy()
    assert (text[16 * n:] == canary).all() and (length[n:] == canary).all()
    return text[:16 * n].reshape(n, 16), length[:n]


def _compare(patterns, want):
    text, length = _float_text(patterns)
    slots = np.frombuffer(b"".join(w.ljust(16, b"\0") for w in want), dtype=np.uint8).reshape(len(want), 16)     # zero padded to a slot
    bad = np.nonzero((text != slots).any(axis=1) | (length != np.asarray([len(w) for w in want], dtype=np.uint8)))[0]
    assert not len(bad), "0x%08x: %r (%d), want %r" % (patterns[bad[0]], text[bad[0]].tobytes(), int(length[bad[0]]), want[bad[0]])


def test_float_text_is_the_rule_in_one_launch():
    """hard() + sweep + 2^18 random patterns: about 2 million values, past one grid-stride pass of the kernel's grid"""
    parts = [("hard", F.hard()), ("sweep2", F.sweep(2, 64)), ("random9", F.randoms(9, 1 << 18))]
    patterns = [b for _, p in parts for b in p]
    want = [w for key, p in parts for w in F.rule_texts(key, p)]
    assert len(patterns) > 1024 * 256
    _compare(patterns, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_float_text_small_counts(n):
    patterns = (F.NANS + F.sweep(3, 1))[:n]
    assert len(patterns) == n
    _compare(patterns, [bam.float_g(b) for b in patterns])


def test_float_text_api_and_arguments():
    import torch
    from ribodetector_amd import _native as N
    from ribodetector_amd import bamtags
    patterns = F.sweep(6, 2)
    bits = torch.from_numpy(np.asarray(patterns, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    text, length = bamtags.float_text(bits)
    f_text, f_length = bamtags.float_text(bits.view(torch.float32))
    torch.cuda.synchronize()
    assert text.shape == (len(patterns), 16) and torch.equal(text, f_text) and torch.equal(length, f_length)
    text, length = text.cpu().numpy(), length.cpu().numpy()
    for k, b in enumerate(patterns):
        assert text[k, :length[k]].tobytes() == bam.float_g(b) and not text[k, length[k]:].any()
    L = N.lib()
    assert L.rd_float_text(None, 0, None, None, None) == 0                 # n == 0: a no-op
    P = 0x10000
    for args in ((None, 4, P, P, None), (P, 4, None, P, None), (P, 4, P, None, None), (P, -1, P, P, None), (P, 4, P + 8, P, None)):
        assert L.rd_float_text(*args) == -1 and b"rd_float_text" in L.rd_last_error()


# ---- the splice -------------------------------------------------------------------------------------------------------------------------
def _views(records):
    data = TC.file_data(records)
    recs = list(bam.records(data))
    assert len(recs) == len(records) and not any(r.skipped for r in recs)
    texts = [r.fastq() for r in recs]
    rs = [0]
    for t in texts:
        rs.append(rs[-1] + len(t))
    raw, st = T.view(records)
    return data, b"".join(texts), rs, raw, st


def _want(data, tags, floats=True):
    parts = []
    for r in bam.records(data):
        t = r.fastq()
        at = t.index(b"\n")
        parts.append(t[:at] + bam.tag_comment(data, r.offset, tags, floats=floats)[0] + t[at:])
    starts = [0]
    for p in parts:
        starts.append(starts[-1] + len(p))
    text = b"".join(parts)
    assert text == bam.fastq_text_tagged(data, tags, floats=floats)
    return text, starts, bam.tag_counts(data, tags, floats=floats)


def _t(b, pad=b"\xa5" * 64):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) + pad, dtype=np.uint8).copy()).to(DEV)[:len(b)]


def _splice(text, rs, raw, st, tags, cap=None, canary=None, floats=True):
    import torch
    from ribodetector_amd import bamtags
    n = len(rs) - 1
    d_text, d_raw = _t(text), _t(raw)
    d_rs, d_st = torch.tensor(rs, dtype=torch.int64, device=DEV), torch.tensor(st, dtype=torch.int64, device=DEV)
    cap = len(text) + 5 * len(raw) if cap is None else cap
    out = None
    if canary is not None:
        out = torch.full((((cap + 255) // 256) * 256 + 256,), canary, dtype=torch.uint8, device=DEV)
    out, out_start, info = bamtags.splice(d_text, d_rs, d_raw, d_st, n, tags, cap, out=out, floats=floats)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_start.cpu().tolist(), info.cpu().tolist()


def _check(records, tags, exact_cap=False):
    data, text, rs, raw, st = _views(records)
    want, starts, counts = _want(data, tags)
    assert len(want) <= len(text) + 5 * len(raw)          # (the documented bound holds with floats on)
    out, out_start, info = _splice(text, rs, raw, st, tags, cap=len(want) if exact_cap else None, canary=0x5a)
    assert info[3] == 0 and info[0] == len(records) and info[1] == len(want)
    assert out_start == starts
    got = out[:len(want)].tobytes()
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        r = max(j for j in range(len(starts)) if starts[j] <= k)
        raise AssertionError("record %d differs at byte %d: %r != %r" % (r, k - starts[r], got[starts[r]:starts[r + 1]], want[starts[r]:starts[r + 1]]))
    assert (out[len(want):] == 0x5a).all()
    assert info[4] == counts["malformed_records"] and info[5] == 0 and counts["float_values_skipped"] == 0
    assert info[8:8 + len(tags)] == counts["copied"] and not any(info[8 + len(tags):])
    return counts


@pytest.mark.parametrize("mapping", LANES)
def test_splice_floats_on_the_hand_built_cases(lanes, mapping):
    lanes(mapping)
    cases = [(name, tags, lst, on, False) for name, tags, lst, on, _ in F.tagged_cases()] + [(name, tags, lst, b"", True) for name, tags, lst in F.MALFORMED_CASES]
    for k, (name, tags, lst, want, mal) in enumerate(cases):
        recs = [TC.case_record(0, T.Z(b"CO", b"before")), TC.case_record(k, tags, flag=0x10 if k % 3 == 0 else 4), TC.case_record(2, b"")]
        data, text, rs, raw, st = _views(recs)
        out, out_start, info = _splice(text, rs, raw, st, lst)
        r = list(bam.records(data))[1].fastq()
        at = r.index(b"\n")
        assert out[out_start[1]:out_start[2]].tobytes() == r[:at] + want + r[at:], name
        assert info[3] == 0 and info[4] == (1 if mal else 0) and info[5] == 0, name
    # every case, the existing ones included, in one view against the rule
    every = [c[1] for c in TC.CASES] + [c[1] for c in cases]
    for lst in ([b"qs"], [b"ML", b"RG", b"NM", b"XX", b"XA", b"XH", b"MM", b"CO", b"qs", b"XF", b"rq", b"XS"]):
        c = _check([TC.case_record(k, tags) for k, tags in enumerate(every)], lst)
    assert c["copied"][8] >= 8 and c["copied"][9] >= 4     # (qs and XF are copied now)


@pytest.mark.parametrize("mapping", LANES)
def test_splice_bf_counts(lanes, mapping):
    """B:f arrays around the lane count of both mappings and of 1,000 elements, texts of 1 to 12 bytes, integer tags on both sides"""
    lanes(mapping)
    hard = F.hard()
    pool = hard[:6000:7] + F.NANS + hard[-2000::97]
    by_len = {}
    for b in pool:
        by_len.setdefault(len(bam.float_g(b)), b)
    assert sorted(by_len) == list(range(1, 13))
    recs = []
    for L in (4, 16):
        for n in (0, 1, L - 1, L, L + 1, 2 * L + 3, 1000):
            vals = [by_len[1 + (5 * i + n) % 12] if i % 3 else pool[(11 * i + n) % len(pool)] for i in range(n)]
            recs.append(T.rec(T.scalar(b"NM", "i", n) + F.bf_tag(b"XF", vals) + T.B(b"ML", "C", [1, 22, 255]) + F.f_tag(b"qs", pool[n % len(pool)]) + T.Z(b"RG", b"behind"),
                              name=b"bf%d_%d" % (L, n)))
    _check(recs, [b"NM", b"XF", b"ML", b"qs", b"RG"])


@pytest.mark.parametrize("mapping", LANES)
@pytest.mark.parametrize("n_rec", [1, 63, 64, 65, 257, 3000])
def test_splice_floats_record_counts(lanes, mapping, n_rec):
    lanes(mapping)
    base, lst = TC.random_records(11, 97)
    c = _check([base[(5 * k + n_rec) % len(base)] for k in range(n_rec)], lst, exact_cap=True)
    if n_rec >= 257:
        assert c["copied"][6] > 10 and c["copied"][7] > 10       # (qs and XF: the random records carry f and B:f values)


@pytest.mark.parametrize("mapping", LANES)
def test_splice_floats_every_output_residue(lanes, mapping):
    """read names of 1..16 bytes, three times over: the float text starts at every residue of the output offset modulo 16"""
    lanes(mapping)
    hard = F.hard()
    recs = [T.rec(F.f_tag(b"qs", hard[(37 * (16 * rep + n)) % 5000]) + F.bf_tag(b"XF", hard[100 * n:100 * n + rep]), name=b"n" * n, seq="ACGT" * (2 + n % 3))
            for rep in range(3) for n in range(1, 17)]
    data, text, rs, raw, st = _views(recs)
    _, starts, _ = _want(data, [b"qs", b"XF"])
    assert set((s + 1 + len(b"n" * n) + 6) % 16 for s, n in zip(starts, [n for _ in range(3) for n in range(1, 17)])) == set(range(16))
    _check(recs, [b"qs", b"XF"])


def test_splice_floats_fault_contract(lanes):
    lanes(None)
    recs, lst = TC.random_records(9, 300)
    data, text, rs, raw, st = _views(recs)
    want, starts, counts = _want(data, lst)
    off = _want(data, lst, floats=False)[0]
    assert len(want) > len(off) > len(text)
    out, out_start, info = _splice(text, rs, raw, st, lst, cap=len(want) - 1, canary=0x5a)
    assert info[3] == 1 and info[1] == len(want) and (out == 0x5a).all()
    assert info[4] == counts["malformed_records"] and info[5] == 0 and info[8:8 + len(lst)] == counts["copied"]
    out, out_start, info2 = _splice(text, rs, raw, st, lst, cap=info[1], canary=0x5a)
    assert info2[3] == 0 and out[:len(want)].tobytes() == want and out_start == starts and (out[len(want):] == 0x5a).all()


def test_splice_ex_without_flags_is_the_splice(lanes):
    """rd_bam_tag_splice_ex with flags = 0 and rd_bam_tag_splice: the same bytes, tables and info; an unknown flag bit is refused"""
    import torch
    from ribodetector_amd import _native as N
    lanes(None)
    recs, lst = TC.random_records(13, 500)
    data, text, rs, raw, st = _views(recs)
    n, cap = len(recs), len(text) + 5 * len(raw)
    d_text, d_raw = _t(text), _t(raw)
    d_rs, d_st = torch.tensor(rs, dtype=torch.int64, device=DEV), torch.tensor(st, dtype=torch.int64, device=DEV)
    L = N.lib()
    ws = torch.empty(int(L.rd_bam_tag_splice_workspace_bytes(n, len(lst))), dtype=torch.uint8, device=DEV)
    res = []
    for flags in (None, 0, 2, 0x80000001):
        out = torch.full((cap + 256,), 0x5a, dtype=torch.uint8, device=DEV)
        out_start = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
        info = torch.full((24,), -7, dtype=torch.int64, device=DEV)
        args = (N.ptr(d_text), len(text), N.ptr(d_rs), N.ptr(d_raw), len(raw), N.ptr(d_st), n, b"".join(lst), len(lst), N.ptr(out), cap, N.ptr(out_start),
                N.ptr(info), N.ptr(ws), ws.numel())
        with torch.cuda.device(DEV):
            rc = L.rd_bam_tag_splice(*args, N.stream_ptr(torch.device(DEV))) if flags is None else L.rd_bam_tag_splice_ex(*args, flags, N.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        if flags in (None, 0):
            assert rc == 0
            res.append((out.cpu().numpy().tobytes(), out_start.cpu().tolist(), info.cpu().tolist()))
        else:                                             # refused without a launch: nothing was written
            assert rc == -1 and b"flag" in L.rd_last_error()
            assert (out == 0x5a).all() and (out_start == -7).all() and (info == -7).all()
    assert res[0] == res[1] and res[0][2][5] > 50 and res[0][0][:res[0][2][1]] == _want(data, lst, floats=False)[0]


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------
LIST = [b"qs", b"XF", b"RG"]


def _cli_records():
    hard = F.hard()
    out = []
    for i in range(400):
        tags = T.Z(b"RG", b"grp%d" % (i % 3)) + T.scalar(b"NM", "i", i)
        if i % 2 == 0:
            tags = F.f_tag(b"qs", F.bits_of(5.0 + (i * 37 % 3500) / 100.0) if i % 8 else hard[(i * 13) % 4000]) + tags
        if i % 5 == 0:
            tags += F.bf_tag(b"XF", hard[i:i + i % 7])
        if i % 41 == 0:
            tags = tags[:len(tags) - 2]                    # a cut tag: malformed
        if i % 43 == 0:
            tags = b"XQq\x01" + tags                       # an unknown type in front: malformed
        seq = "".join("ACGT"[(i * 7 + j * j + j // 3) % 4] for j in range(40 + i % 21))
        out.append(T.rec(tags, name=b"read%d" % i, seq=seq, flag=0x10 if i % 9 == 0 else 4))
    return out


def _read(path):
    with open(path, "rb") as fh:
        raw = fh.read()
    return gzip.decompress(raw) if path.endswith("gz") else raw


def _records_of(text):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


@pytest.mark.parametrize("floats", [True, False])
def test_cli_bam_tag_floats(caplog, tmp_path, floats):
    """the two outputs together are the records of the rule, each in one file and in input order; the summary and the log line say what
    was copied. Without the flag (floats=False) the same run gives what it gave before the flag existed."""
    import logging
    import test_gpu_bam as G
    caplog.set_level(logging.INFO)
    path = str(tmp_path / "x.bam")
    data = bam.write_bam(path, _cli_records())
    files = [str(tmp_path / f) for f in ("non.fq", "rrna.fq.gz", "s.json")]
    G._run(["-l", "100", "-i", path, "-o", files[0], "-r", files[1], "--bam_tags", "qs,XF,RG", "--summary", files[2]] + (["--bam_tag_floats"] if floats else []) + G.SMALL)
    kw = {"floats": True} if floats else {}                # (without the flag: the calls as they were before the keyword existed)
    want = _records_of(bam.fastq_text_tagged(data, LIST, **kw))
    got = [_records_of(_read(f)) for f in files[:2]]
    assert len(want) == 400 and len(got[0]) + len(got[1]) == 400
    at = [0, 0]
    for w in want:                                        # every record in one of the two files, in input order
        k = 0 if at[0] < len(got[0]) and got[0][at[0]] == w else 1
        assert at[k] < len(got[k]) and got[k][at[k]] == w, w
        at[k] += 1
    counts = bam.tag_counts(data, LIST, **kw)
    doc = json.load(open(files[2]))["bam_tags"]
    expect = dict({"tags": [t.decode() for t in LIST]}, **counts)
    if floats:
        expect["float_format"] = "%g"
        assert list(doc)[-1] == "float_format"
    assert doc == expect
    assert counts["malformed_records"] >= 10 and (counts["float_values_skipped"] == 0) == floats
    if floats:
        assert counts["copied"][0] > 150 and counts["copied"][1] > 50 and b"\tqs:f:" in b"".join(want) and b"\tXF:B:f," in b"".join(want)
    line = [m for m in caplog.messages if m.startswith("BAM tags: ")]
    assert len(line) == 1 and line[0].endswith("%d float values skipped" % counts["float_values_skipped"])
    assert line[0] == "BAM tags: qs %d, XF %d, RG %d copied; %d records with malformed tags, %d float values skipped" % (
        *counts["copied"], counts["malformed_records"], counts["float_values_skipped"])
